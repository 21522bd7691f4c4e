"""mmc_featureset_knn on the MI355X (csrc/neighbors.hip, mermaid_classifier_amd/neighbors.py) against the float64 checker of
tests/neighbors_checker.py, per query, at the smallest shapes that reach every edge: one row, one below / exactly / one above a
tile, several tiles with a ragged one, every split holding two base tiles, two query tiles, a query chunk boundary, the production
width, k above the number of eligible rows, ranges that start inside their sets with decoys around them, negative scores (a padding
row's 0 would win), a self-search with a knocked-out base tile, and integer inputs whose ties must come out in row order bit for bit.
The bounds are derived in the checker's header; every gate is 1 x.  Worst score error / bound on an MI355X: profiles/knn.txt."""

import numpy as np
import pytest

import neighbors_checker as ck

pytestmark = pytest.mark.gpu

K_CLASSES = 4
FQ, FB = ck.FIRST_Q, ck.FIRST_B


def _set(X, y, K=K_CLASSES):
    from mermaid_classifier_amd import FeatureSet
    return FeatureSet(X.shape[1], np.arange(K)).append(X, y)


@pytest.fixture(scope="module")
def bounded():
    """per dim: the two sets on the device, their host rows, and a cache of float64 references"""
    made = {}

    def get(dim, nb_max=ck.NB_MAX):
        if (dim, nb_max) not in made:
            Xq, yq, Xb, yb = ck.bounded_inputs(dim, seed=10 * dim, nb_max=nb_max)
            made[dim, nb_max] = dict(Xq=Xq, yq=yq, Xb=Xb, yb=yb, q=_set(Xq, yq), b=_set(Xb, yb), ref={})
        return made[dim, nb_max]

    yield get
    for m in made.values():
        m["q"].close()
        m["b"].close()


def _reference(m, metric, nq, nb):
    if (metric, nq, nb) not in m["ref"]:
        m["ref"][metric, nq, nb] = ck.reference(m["Xq"][FQ:FQ + nq], m["Xb"][FB:FB + nb], metric)
    return m["ref"][metric, nq, nb]


def _check_labels(nb_out, yb_range):
    ok = nb_out.index >= 0
    assert np.array_equal(nb_out.label[ok], yb_range[nb_out.index[ok]]) and np.all(nb_out.label[~ok] == -1)


@pytest.mark.parametrize("dim", [8, 72])
@pytest.mark.parametrize("metric", [ck.DOT, ck.COSINE, ck.L2])
def test_ranges_with_decoys_every_tile_edge(bounded, dim, metric):
    from mermaid_classifier_amd import nearest
    m = bounded(dim)
    name = ck.METRIC_NAMES[metric]
    worst = 0.0
    for nq in (1, 129):
        for nb in (1, 127, 128, 129, 700):
            s64, beta = _reference(m, metric, nq, nb)
            elig = ck.eligibility(nq, nb)
            if nq == 129 and metric != ck.L2:
                assert (s64[64:] < 0).mean() > 0.99                                    # a padding row's 0 would head these lists
            for k in (1, 5, 32):
                got = nearest(m["q"], m["b"], k, name, query_rows=(FQ, nq), base_rows=(FB, nb))
                worst = max(worst, ck.accept(got.index, got.score, s64, beta, elig, k, f"dim {dim} {name} nq {nq} nb {nb} k {k}"))
                _check_labels(got, m["yb"][FB:FB + nb])
                if k == 5:
                    again = nearest(m["q"], m["b"], k, name, query_rows=(FQ, nq), base_rows=(FB, nb))
                    assert np.array_equal(got.index, again.index) and np.array_equal(got.score.view(np.uint32), again.score.view(np.uint32))
                    if nq == 129:                                                      # another query range: the same lists
                        part = nearest(m["q"], m["b"], k, name, query_rows=(FQ + 100, 29), base_rows=(FB, nb))
                        assert np.array_equal(part.index, got.index[100:]) and np.array_equal(part.score.view(np.uint32), got.score[100:].view(np.uint32))
    print(f"knn dim {dim} {name}: worst |score - float64| / bound {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("metric", [ck.DOT, ck.COSINE, ck.L2])
def test_every_split_holds_two_base_tiles(bounded, metric):
    from mermaid_classifier_amd import nearest
    from mermaid_classifier_amd.neighbors import knn_splits
    nb = ck.NB_TWO_TILES
    assert knn_splits(129, nb) == ck.MAX_SPLITS and -(-nb // ck.TILE) == 2 * ck.MAX_SPLITS
    m = bounded(8, nb)
    s64, beta = _reference(m, metric, 129, nb)
    got = nearest(m["q"], m["b"], 5, ck.METRIC_NAMES[metric], query_rows=(FQ, 129), base_rows=(FB, nb))
    worst = ck.accept(got.index, got.score, s64, beta, ck.eligibility(129, nb), 5, f"two tiles per split, {ck.METRIC_NAMES[metric]}")
    print(f"knn dim 8 {ck.METRIC_NAMES[metric]} nb {nb}: worst |score - float64| / bound {worst:.3g}")
    one = nearest(m["q"], m["b"], 5, ck.METRIC_NAMES[metric], query_rows=(FQ + 7, 1), base_rows=(FB, nb))   # one query tile, other splits
    assert np.array_equal(one.index, got.index[7:8]) and np.array_equal(one.score.view(np.uint32), got.score[7:8].view(np.uint32))


@pytest.mark.parametrize("metric", [ck.DOT, ck.COSINE, ck.L2])
def test_production_width(bounded, metric):
    from mermaid_classifier_amd import nearest
    Xq, yq, Xb, yb = ck.bounded_inputs(1280, seed=5, nb_max=300)
    q, b = _set(Xq, yq), _set(Xb, yb)
    try:
        s64, beta = ck.reference(Xq[FQ:FQ + 129], Xb[FB:FB + 300], metric)
        got = nearest(q, b, 5, ck.METRIC_NAMES[metric], query_rows=(FQ, 129), base_rows=(FB, 300))
        worst = ck.accept(got.index, got.score, s64, beta, ck.eligibility(129, 300), 5, f"dim 1280 {ck.METRIC_NAMES[metric]}")
        print(f"knn dim 1280 {ck.METRIC_NAMES[metric]}: worst |score - float64| / bound {worst:.3g}")
    finally:
        q.close()
        b.close()


def test_odd_width_takes_the_scalar_staging():
    """dim = 10 is no multiple of 4: the staging loads element by element, and the last stage is ragged"""
    from mermaid_classifier_amd import nearest
    Xq, yq, Xb, yb = ck.bounded_inputs(10, seed=9, nb_max=300)
    q, b = _set(Xq, yq), _set(Xb, yb)
    try:
        for metric in (ck.DOT, ck.COSINE, ck.L2):
            s64, beta = ck.reference(Xq[FQ:FQ + 129], Xb[FB:FB + 300], metric)
            got = nearest(q, b, 5, ck.METRIC_NAMES[metric], query_rows=(FQ, 129), base_rows=(FB, 300))
            ck.accept(got.index, got.score, s64, beta, ck.eligibility(129, 300), 5, f"dim 10 {ck.METRIC_NAMES[metric]}")
    finally:
        q.close()
        b.close()


def test_self_search_groups_knock_out_a_base_tile_host_and_device_outputs():
    """query == base on overlapping ranges with EXCLUDE_SELF; the queries of group 7 lose base tile 1 whole.  Through the raw ABI,
    device outputs with device groups give the bits of host outputs with host groups.  With 20 base rows k = 32 outruns the eligible
    rows and the tail is filled."""
    import torch
    from mermaid_classifier_amd import _lib, nearest
    X, y = ck.clustered(400, 8, K_CLASSES, seed=3, negate_from=200)
    fs = _set(X, y)
    q_first, nq, b_first, nb, k = 10, 129, 4, 300, 32
    bg = (np.arange(nb) % 5).astype(np.int32)
    bg[128:256] = 7
    qg = np.where(np.arange(nq) % 3 == 0, 7, 100 + np.arange(nq)).astype(np.int32)
    elig = ck.eligibility(nq, nb, qg, bg, q_first - b_first)
    lib = _lib.lib()
    try:
        for metric in (ck.DOT, ck.COSINE, ck.L2):
            s64, beta = ck.reference(X[q_first:q_first + nq], X[b_first:b_first + nb], metric)
            got = nearest(fs, fs, k, ck.METRIC_NAMES[metric], query_groups=qg, base_groups=bg, exclude_self=True,
                          query_rows=(q_first, nq), base_rows=(b_first, nb))
            ck.accept(got.index, got.score, s64, beta, elig, k, f"self-search {ck.METRIC_NAMES[metric]}")
            assert not np.isin(got.index[0], np.arange(128, 256)).any() and not (got.index[1] == 7).any()
            _check_labels(got, y[b_first:b_first + nb])
            d_qg, d_bg = torch.from_numpy(qg).cuda(), torch.from_numpy(bg).cuda()
            d_index = torch.full((nq, k), 77, dtype=torch.int32, device="cuda")
            d_score = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
            d_label = torch.full((nq, k), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            _lib.check(lib.mmc_featureset_knn(fs._handle(), q_first, nq, fs._handle(), b_first, nb, k, metric, d_qg.data_ptr(), d_bg.data_ptr(),
                                              d_index.data_ptr(), d_score.data_ptr(), d_label.data_ptr(), _lib.MMC_KNN_EXCLUDE_SELF, None))
            assert np.array_equal(d_index.cpu().numpy(), got.index) and np.array_equal(d_label.cpu().numpy(), got.label)
            assert np.array_equal(d_score.cpu().numpy().view(np.uint32), got.score.view(np.uint32))
        # 20 base rows, k = 32, one group out: the tail is filled
        short = nearest(fs, fs, 32, "l2", query_groups=qg[:5], base_groups=bg[:20], exclude_self=True, query_rows=(q_first, 5), base_rows=(b_first, 20))
        s64, beta = ck.reference(X[q_first:q_first + 5], X[b_first:b_first + 20], ck.L2)
        ck.accept(short.index, short.score, s64, beta, ck.eligibility(5, 20, qg[:5], bg[:20], q_first - b_first), 32, "short lists")
        assert (short.index[:, -1] == -1).all() and (short.label[:, -1] == -1).all()
    finally:
        fs.close()


def test_integer_inputs_match_float64_bit_for_bit():
    from mermaid_classifier_amd import nearest
    X, y = ck.integer_rows(450, 8, seed=1)
    fs = _set(X, y)
    try:
        for metric in (ck.DOT, ck.L2):
            for nq, nb, k in ((129, 300, 5), (129, 129, 32), (1, 127, 1), (129, 428, 32)):
                s64, _ = ck.reference(X[2:2 + nq], X[20:20 + nb], metric)
                elig = ck.eligibility(nq, nb, self_shift=2 - 20)
                got = nearest(fs, fs, k, ck.METRIC_NAMES[metric], exclude_self=True, query_rows=(2, nq), base_rows=(20, nb))
                ck.assert_exact(got.index, got.score, s64, elig, k, f"{ck.METRIC_NAMES[metric]} {nq} x {nb} k {k}")
    finally:
        fs.close()


def test_nan_orders_below_every_number():
    from mermaid_classifier_amd import nearest
    X, y = ck.integer_rows(40, 8, seed=6)
    X[5, 3] = np.nan
    X[9] = 0                                                         # a zero row: cosine 0 against everything
    fs = _set(X, y)
    try:
        for metric in ("dot", "cosine"):
            got = nearest(fs, fs, 32, metric, query_rows=(20, 4), base_rows=(0, 12))
            assert np.all(got.index[:, 11] == 5) and np.all(np.isnan(got.score[:, 11])) and np.all(got.index[:, 12:] == -1)
            assert np.all(np.isfinite(got.score[:, :11])) and np.all(np.diff(got.score[:, :11], axis=1) <= 0)
        zero = nearest(fs, fs, 3, "cosine", query_rows=(9, 1), base_rows=(0, 5))
        assert zero.index.tolist() == [[0, 1, 2]] and not zero.score.any() and not np.signbit(zero.score).any()
    finally:
        fs.close()


def test_a_query_chunk_boundary():
    """nq just above MMC_KNN_CHUNK_ROWS: the second chunk's queries get the lists a call on them alone gets"""
    from mermaid_classifier_amd import nearest
    n = ck.CHUNK + 129
    Xq, yq = ck.clustered(n, 8, K_CLASSES, seed=12, negate_from=n // 2)
    Xb, yb = ck.clustered(300, 8, K_CLASSES, seed=13)
    q, b = _set(Xq, yq), _set(Xb, yb)
    try:
        full = nearest(q, b, 5, "cosine")
        first = ck.CHUNK - 60
        part = nearest(q, b, 5, "cosine", query_rows=(first, n - first))
        assert np.array_equal(full.index[first:], part.index) and np.array_equal(full.score[first:].view(np.uint32), part.score.view(np.uint32))
        s64, beta = ck.reference(Xq[first:], Xb, ck.COSINE)
        ck.accept(part.index, part.score, s64, beta, ck.eligibility(n - first, 300), 5, "chunk boundary")
    finally:
        q.close()
        b.close()


def test_argument_errors_and_empty_ranges():
    from mermaid_classifier_amd import FeatureSet, _lib
    X, y = ck.integer_rows(30, 8, seed=2)
    a, b = _set(X, y), _set(X[:10], y[:10])
    wide = FeatureSet(9, np.arange(K_CLASSES)).append(np.zeros((3, 9), np.float32), [0, 1, 2])
    lib = _lib.lib()
    index = np.full((30, 32), 55, np.int32)
    score = np.full((30, 32), 55, np.float32)
    label = np.full((30, 32), 55, np.int32)
    g = np.zeros(30, np.int32)
    H = _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST

    def call(q=a, qf=0, nq=5, bs=b, bf=0, nb=10, k=3, metric=0, qg=None, bg=None, idx=index, sc=score, flags=H):
        return lib.mmc_featureset_knn(q._handle() if q is not None else None, qf, nq, bs._handle() if bs is not None else None, bf, nb, k, metric,
                                      None if qg is None else qg.ctypes.data, None if bg is None else bg.ctypes.data,
                                      None if idx is None else idx.ctypes.data, None if sc is None else sc.ctypes.data, label.ctypes.data, flags, None)

    bad = [(dict(qf=28, nq=5), "outside the set's"), (dict(bf=-1), "outside the set's"), (dict(nb=11), "outside the set's"),
           (dict(nq=-1), "outside the set's"), (dict(k=0), "MMC_KNN_MAX_K"), (dict(k=33), "MMC_KNN_MAX_K"), (dict(metric=3), "metric"),
           (dict(metric=-1), "metric"), (dict(flags=H | 8), "flags"), (dict(flags=H | _lib.MMC_KNN_EXCLUDE_SELF), "same set"),
           (dict(qg=g), "both, or neither"), (dict(bg=g), "both, or neither"), (dict(bs=wide, nb=3), "width"), (dict(idx=None), "NULL"),
           (dict(sc=None), "NULL"), (dict(q=None), "NULL"), (dict(bs=None), "NULL")]
    for kwargs, match in bad:
        assert call(**kwargs) == _lib.MMC_ERR_ARG, kwargs
        assert match in lib.mmc_last_error().decode(), (kwargs, lib.mmc_last_error().decode())
    assert (index == 55).all() and (score == 55).all() and (label == 55).all()        # a rejected call writes nothing
    assert call(nq=0) == _lib.MMC_OK and (index == 55).all()                          # no queries: nothing written
    assert call(nq=5, nb=0, k=4) == _lib.MMC_OK                                        # no base rows: the tail values
    assert (index.ravel()[:20] == -1).all() and np.isneginf(score.ravel()[:20]).all() and (label.ravel()[:20] == -1).all()
    assert (index.ravel()[20:] == 55).all()
    assert call(q=a, bs=a, nq=30, nb=30, k=32, flags=H | _lib.MMC_KNN_EXCLUDE_SELF) == _lib.MMC_OK   # a legal self-search
    assert (index[:, :29] >= 0).all() and (index[:, 29:] == -1).all() and not (index == np.arange(30)[:, None]).any()
    for fs in (a, b, wide):
        fs.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_knn_validate_and_audit_labels_end_to_end():
    from mermaid_classifier_amd import FeatureSet, audit_labels, knn_validate, near_duplicates
    from mermaid_classifier_amd.neighbors import Neighbors, confusion_table
    dim, K, k = 16, 5, 5
    Xt, yt = ck.clustered(600, dim, K, seed=60)
    Xv, yv = ck.clustered(200, dim, K, seed=61)
    Xv[:4] = Xt[[10, 20, 30, 40]]                                    # four validation rows leaked from the training split
    classes = np.array([2, 3, 5, 7, 11])
    train = FeatureSet(dim, classes).append(Xt, classes[yt])
    val = FeatureSet(dim, classes).append(Xv, classes[yv])
    try:
        s64, beta = ck.reference(Xv, Xt, ck.COSINE)
        elig = ck.eligibility(200, 600)
        assert ck.ambiguous_share(s64, beta, elig, k) == 0            # the reference's lists are settled: the tables must be equal
        r_index, _ = ck.reference_topk(s64, elig, k)
        r_est = Neighbors(r_index, np.zeros_like(r_index, np.float32), yt[r_index], classes).votes().argmax(1)
        sources = np.arange(200) % 3
        res = knn_validate(train, val, k, sources=sources)
        assert np.array_equal(res.confusion, confusion_table(yv, r_est, K)) and res.confusion.sum() == 200
        assert res.scores.confusion is not res.confusion and res.scores.accuracy == float((r_est == yv).mean())
        acc = [float((r_est == yv)[sources == s].mean()) for s in range(3)]
        assert res.sources.scalars() == {"per_source/n_sources": 3.0, "per_source/min_accuracy": min(acc), "per_source/max_accuracy": max(acc)}
        print(f"knn probe: accuracy {res.scores.accuracy:.3f}, balanced {res.scores.balanced_accuracy:.3f}, per source {acc}")
        dup = near_duplicates(val, train, 0.9999)
        assert dup["a"].tolist() == [0, 1, 2, 3] and dup["b"].tolist() == [10, 20, 30, 40]
    finally:
        train.close()
        val.close()
    # label audit: well-separated clusters, 12 labels flipped on purpose, 4 points per image
    rng = np.random.default_rng(2)
    centres = 4 * rng.normal(0, 1, (K, dim))
    y = rng.integers(0, K, 400)
    X = (centres[y] + 0.3 * rng.normal(0, 1, (400, dim))).astype(np.float32)
    flipped = np.sort(rng.choice(400, 12, replace=False))
    noisy = y.copy()
    noisy[flipped] = (y[flipped] + 1 + rng.integers(0, K - 1, 12)) % K
    fs = FeatureSet(dim, classes).append(X, classes[noisy])
    try:
        table = audit_labels(fs, 8, groups=np.arange(400) // 4)
        assert sorted(table["row"][:12].tolist()) == flipped.tolist()
        assert np.array_equal(table["majority"][:12], classes[y[table["row"][:12]]]) and table["agreement"][:12].max() < 0.5
        assert table["agreement"][12:].min() > 0.5 and np.all(np.diff(table["agreement"]) >= 0)
        plain = audit_labels(fs, 8)
        assert sorted(plain["row"][:12].tolist()) == flipped.tolist()
    finally:
        fs.close()
