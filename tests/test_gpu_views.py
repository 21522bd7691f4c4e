"""-m gpu: patch views (include/mmc.h, "patch views") through the C ABI and the Python front-ends.

Every comparison is bit for bit: patches against the numpy definition of tests/views_checker.py (the reference's own crop, the
integer 2:1 reduction, np.rot90), the view-averaged top-k against a left-to-right fp32 mean of the same handle's
mmc_head_predict rows followed by a stable host sort, and the fused routes against the routes a user composes."""

import numpy as np
import pytest

import views_checker as vc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

POINTS_SMALL = [(0, 0), (0, 240), (228, 0), (228, 240), (114, 120), (3, 237)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _load(name):
    from mermaid_classifier_amd import load_predictor
    return load_predictor(GOLDEN / name / "model.pt", GOLDEN / name / "model.json")


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(2024)
    return (rng.integers(0, 256, (229, 241, 3), dtype=np.uint8),      # both sides > 224, odd, no multiples of 4
            rng.integers(0, 256, (640, 600, 3), dtype=np.uint8))


@pytest.fixture(scope="module")
def want_small(images):
    """view_patch of every (point, view) of the small image: [point][view], computed once."""
    return [[vc.view_patch(images[0], r, c, v) for v in range(16)] for r, c in POINTS_SMALL]


@pytest.fixture(scope="module")
def want_big(images):
    return {(r, c): [vc.view_patch(images[1], r, c, v) for v in range(16)] for r, c in ((0, 599), (320, 300))}


def crop_views(image, rowcols, codes, on_device=False, plain=False):
    """mmc_crop_patches_views (mmc_crop_patches when ``plain``) -> (n, 224, 224, 3) uint8 host array.  codes None = NULL."""
    import torch
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    rc = np.ascontiguousarray(np.asarray(rowcols, np.int32).reshape(-1, 2))
    n = len(rc)
    cd = None if codes is None else np.ascontiguousarray(np.asarray(codes, np.uint8))
    assert cd is None or len(cd) == n
    out = torch.zeros((n, 224, 224, 3), dtype=torch.uint8, device="cuda:0")
    stream = int(torch.cuda.current_stream(0).cuda_stream)
    if on_device:
        im_d, rc_d = torch.from_numpy(image).cuda(), torch.from_numpy(rc).cuda()
        cd_d = None if cd is None else torch.from_numpy(cd).cuda()
        ptrs, flags = (im_d.data_ptr(), rc_d.data_ptr(), None if cd is None else cd_d.data_ptr()), 0
    else:
        ptrs, flags = (image.ctypes.data, rc.ctypes.data, None if cd is None else cd.ctypes.data), _lib.MMC_IN_HOST
    if plain:
        assert cd is None
        _lib.check(lib.mmc_crop_patches(ptrs[0], image.shape[0], image.shape[1], ptrs[1], n, out.data_ptr(), flags, 0, stream))
    else:
        _lib.check(lib.mmc_crop_patches_views(ptrs[0], image.shape[0], image.shape[1], ptrs[1], n, ptrs[2], out.data_ptr(), flags, 0,
                                              stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. crop, kernel path ----

@pytest.mark.parametrize("on_device", [False, True])
def test_crop_views_kernel_path_is_view_patch(images, want_small, on_device):
    """96 patches on a 229x241 image (6 points x 16 views: upload + kernel under host arguments, the kernel alone under device
    arguments), corners included."""
    rc = [p for p in POINTS_SMALL for _ in range(16)]
    codes = list(range(16)) * len(POINTS_SMALL)
    got = crop_views(images[0], rc, codes, on_device=on_device)
    for i, p in enumerate(POINTS_SMALL):
        for v in range(16):
            assert np.array_equal(got[i * 16 + v], want_small[i][v]), (p, v)


# ---- 2. crop, host-cut path ----

def test_crop_views_host_cut_and_upload_agree(images, want_big):
    """640x600: one patch per call is cut on the host (1 * 150528 * 6 <= 1152000 image bytes), two or more are uploaded and cut
    by the kernel.  No environment variable is set."""
    import os
    assert "MMC_CROP_HOST" not in os.environ
    im = images[1]
    pts = list(want_big)
    assert 1 * 150528 * 6 <= im.nbytes < 2 * 150528 * 6
    kernel = crop_views(im, [p for p in pts for _ in range(16)], list(range(16)) * 2)
    for i, p in enumerate(pts):
        for v in range(16):
            host = crop_views(im, [p], [v])[0]
            assert np.array_equal(host, want_big[p][v]), (p, v)
            assert np.array_equal(kernel[i * 16 + v], want_big[p][v]), (p, v)


# ---- 3. the plain route is unchanged ----

def test_null_views_and_all_zero_views_are_mmc_crop_patches(images, want_small, want_big):
    small, big = images
    for on_device in (False, True):
        plain = crop_views(small, POINTS_SMALL, None, on_device=on_device, plain=True)
        assert np.array_equal(plain, np.stack([w[0] for w in want_small]))
        assert np.array_equal(crop_views(small, POINTS_SMALL, None, on_device=on_device), plain)
        assert np.array_equal(crop_views(small, POINTS_SMALL, [0] * len(POINTS_SMALL), on_device=on_device), plain)
    pts = list(want_big)
    for sel in ([pts[0]], [pts[1]], pts):                               # host cut, host cut, upload + kernel
        plain = crop_views(big, sel, None, plain=True)
        assert np.array_equal(plain, np.stack([want_big[p][0] for p in sel]))
        assert np.array_equal(crop_views(big, sel, None), plain)
        assert np.array_equal(crop_views(big, sel, [0] * len(sel)), plain)


# ---- 4. device codes are masked ----

def test_device_view_codes_are_masked_to_four_bits(images, want_small):
    got = crop_views(images[0], [POINTS_SMALL[5], POINTS_SMALL[4]], [16 + 5, 0xF0 | 9], on_device=True)
    assert np.array_equal(got[0], want_small[5][5]) and np.array_equal(got[1], want_small[4][9])
    with pytest.raises(ValueError, match="view code 21 of patch 0"):   # the same code in host memory is refused
        crop_views(images[0], [POINTS_SMALL[5]], [21])


# ---- 5. mean top-k on features ----

@pytest.mark.parametrize("name", ["head_fixture", "head108"])
@pytest.mark.parametrize("on_device", [False, True])
def test_mean_topk_is_the_checker_on_predict_rows(name, on_device):
    import torch
    head = _load(name)._head
    K = head.n_classes
    rng = np.random.default_rng(7)
    P = 7                                                                # not a multiple of the 4 points per workgroup
    for G in (1, 3, 8, 16):
        X = rng.normal(0.3, 0.6, (P * G, head.input_dim)).astype(np.float32)
        proba, _ = head.predict(X)
        xin = torch.from_numpy(X).cuda() if on_device else X
        for k in (1, 5, K):
            want_i, want_s, want_m = vc.mean_topk(proba, G, k)
            idx, sc, pr = head.topk(xin, k, want_proba=True, views_per_point=G)
            idx2, sc2 = head.topk(xin, k, views_per_point=G)
            if on_device:
                torch.cuda.synchronize()
                idx, sc, pr, idx2, sc2 = (t.cpu().numpy() for t in (idx, sc, pr, idx2, sc2))
            assert idx.shape == (P, k) and idx.dtype == np.int32 and sc.dtype == np.float32 and pr.shape == (P, K)
            assert np.array_equal(idx, want_i) and np.array_equal(bits(sc), bits(want_s)), (G, k)
            assert np.array_equal(bits(pr), bits(want_m)), (G, k)
            assert np.array_equal(idx2, want_i) and np.array_equal(bits(sc2), bits(want_s)), (G, k)
            if G == 1:                                                   # the bits of mmc_head_topk
                ti, ts = head.topk(X, k)
                assert np.array_equal(idx, ti) and np.array_equal(bits(sc), bits(ts)) and np.array_equal(bits(pr), bits(proba))


# ---- 6. a head wider than the LDS row ----

def test_mean_topk_of_a_head_wider_than_the_lds_row():
    """K = 2100 > TOPK_LDS_MAX_K: the mean row lives in global memory (the probability output, or the scratch rows)."""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(5)
    K, G, P = 2100, 3, 9
    prm = HeadParams([rng.normal(0, 0.5, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                     rng.uniform(-30, -5, K).astype(np.float32), rng.uniform(1, 4, K).astype(np.float32))
    head = DeviceHead(prm)
    X = rng.normal(0, 1, (P * G, 8)).astype(np.float32)
    proba, _ = head.predict(X)
    for k in (1, 5, 70):
        want_i, want_s, want_m = vc.mean_topk(proba, G, k)
        idx, sc = head.topk(X, k, views_per_point=G)
        assert np.array_equal(idx, want_i) and np.array_equal(bits(sc), bits(want_s))
        idx, sc, pr = head.topk(X, k, want_proba=True, views_per_point=G)
        assert np.array_equal(idx, want_i) and np.array_equal(bits(sc), bits(want_s)) and np.array_equal(bits(pr), bits(want_m))
    head.close()


# ---- 6b. G = 1 through the views entries themselves ----

def _abi_topk(head, X, k, G, on_device, views_entry, with_proba=True):
    """mmc_head_topk_views (or mmc_head_topk when not ``views_entry``) called through the C ABI, no Python routing in between
    -> (idx, scores, proba) host arrays."""
    import torch
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    P, K = len(X) // G, head.n_classes
    stream = int(torch.cuda.current_stream(0).cuda_stream)
    if on_device:
        xd = torch.from_numpy(X).cuda()
        i = torch.full((P, k), -1, dtype=torch.int32, device="cuda")
        s = torch.full((P, k), -1.0, dtype=torch.float32, device="cuda")
        p = torch.full((P, K), -1.0, dtype=torch.float32, device="cuda")
        ptrs, flags = (xd.data_ptr(), i.data_ptr(), s.data_ptr(), p.data_ptr()), 0
    else:
        i, s, p = np.full((P, k), -1, np.int32), np.full((P, k), -1, np.float32), np.full((P, K), -1, np.float32)
        ptrs, flags = (X.ctypes.data, i.ctypes.data, s.ctypes.data, p.ctypes.data), _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST
    if not with_proba:
        ptrs = ptrs[:3] + (None,)
    if views_entry:
        _lib.check(lib.mmc_head_topk_views(head._h, ptrs[0], P, G, k, ptrs[1], ptrs[2], ptrs[3], flags, stream))
    else:
        assert G == 1
        _lib.check(lib.mmc_head_topk(head._h, ptrs[0], P, k, ptrs[1], ptrs[2], ptrs[3], flags, stream))
    torch.cuda.synchronize()
    return (i.cpu().numpy(), s.cpu().numpy(), p.cpu().numpy()) if on_device else (i, s, p)


def _wide_head():
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    rng = np.random.default_rng(5)
    K = 2100
    return DeviceHead(HeadParams([rng.normal(0, 0.5, (K, 8)).astype(np.float32)], [rng.normal(0, 0.1, K).astype(np.float32)],
                                 rng.uniform(-30, -5, K).astype(np.float32), rng.uniform(1, 4, K).astype(np.float32)))


@pytest.mark.parametrize("name", ["head_fixture", "head108", "wide"])
@pytest.mark.parametrize("on_device", [False, True])
def test_one_view_per_point_through_mmc_head_topk_views_has_the_bits_of_mmc_head_topk(name, on_device):
    """mean_topk_kernel launched with G = 1 (the Python wrappers send one view per point to mmc_head_topk, so this goes
    through the C ABI): indices, scores and the probability output equal mmc_head_topk's and the mmc_head_predict rows."""
    head = _wide_head() if name == "wide" else _load(name)._head
    K = head.n_classes
    rng = np.random.default_rng(17)
    X = rng.normal(0.3, 0.6, (7, head.input_dim)).astype(np.float32)
    proba, arg = head.predict(X)
    for k in (1, 5, K):
        vi, vs, vp = _abi_topk(head, X, k, 1, on_device, views_entry=True)
        ti, ts, tp = _abi_topk(head, X, k, 1, on_device, views_entry=False)
        want_i, want_s, want_m = vc.mean_topk(proba, 1, k)
        assert np.array_equal(vi, ti) and np.array_equal(bits(vs), bits(ts)) and np.array_equal(bits(vp), bits(tp)), k
        assert np.array_equal(vi, want_i) and np.array_equal(bits(vs), bits(want_s)) and np.array_equal(bits(vp), bits(proba)), k
        assert np.array_equal(vi[:, 0], arg)
        ni, ns, _ = _abi_topk(head, X, k, 1, on_device, views_entry=True, with_proba=False)     # the row in LDS / the scratch rows
        assert np.array_equal(ni, ti) and np.array_equal(bits(ns), bits(ts)), k
    if name == "wide":
        head.close()


# ---- 7. ties and NaN ----

def _exact(v, G):
    """True where every partial sum j v, j <= G, is an fp32 number, i.e. where (v + v + ... + v) / G, summed left to right, is v."""
    v64 = v.astype(np.float64)
    return np.all([(v64 * j).astype(np.float32).astype(np.float64) == v64 * j for j in range(1, G + 1)], axis=0)


@pytest.mark.parametrize("G", [2, 8])
def test_identical_views_have_the_bits_and_the_order_of_the_single_row(G):
    """G copies of a row.  (v + v + ... + v) / (float)G, summed left to right as the definition says, is v bit for bit exactly
    when every partial sum j v is an fp32 number: always for G = 2; for G = 8 only when v's significand leaves three spare bits
    (3v, 5v, 6v and 7v round otherwise).  So the single row's bits and mmc_head_topk's order are asserted
      - at G = 2 and G = 8 on a head whose rows are exact ties (Platt a = 0, b = -+200: four classes at 1/4, one at 0), and
      - at G = 2 on the fixture with classes 1 and 3 made equal (general 24-bit probabilities);
    at G = 8 those general rows must have the single row's bits wherever the partial sums are exact and the checker's bits
    everywhere, with classes 1 and 3 still tied.  (On these rows the mean of 8 copies differs from the row by 1-2 units in the
    last place in many entries, on the MI355X as in the numpy checker.)"""
    from mermaid_classifier_amd.inference import DeviceHead, HeadParams
    io = np.load(GOLDEN / "head_fixture_io.npz")
    X = io["X"][:23]
    rep = np.repeat(X, G, axis=0)
    # exact ties
    ties = DeviceHead(HeadParams([io["W0"], io["W1"]], [io["b0"], io["b1"]], np.zeros(5, np.float32),
                                 np.array([-200, -200, 200, -200, -200], np.float32)))
    proba, _ = ties.predict(X)
    assert np.all(proba == np.array([0.25, 0.25, 0, 0.25, 0.25], np.float32))
    for k in (2, 5):
        ti, ts = ties.topk(X, k)
        assert np.array_equal(ti, np.tile(np.array([0, 1, 3, 4, 2], np.int32)[:k], (len(X), 1)))
        idx, sc, pr = ties.topk(rep, k, want_proba=True, views_per_point=G)
        assert np.array_equal(idx, ti) and np.array_equal(bits(sc), bits(ts)) and np.array_equal(bits(pr), bits(proba))
    ties.close()
    # general probabilities, two classes tied
    W1, b1, a, b = io["W1"].copy(), io["b1"].copy(), io["a"].copy(), io["b"].copy()
    W1[3], b1[3], a[3], b[3] = W1[1], b1[1], a[1], b[1]
    head = DeviceHead(HeadParams([io["W0"], W1], [io["b0"], b1], a, b))
    proba, _ = head.predict(X)
    assert np.array_equal(bits(proba[:, 1]), bits(proba[:, 3]))
    exact = _exact(proba, G)
    assert exact.all() or G > 2
    for k in (2, 5):
        ti, ts = head.topk(X, k)
        idx, sc, pr = head.topk(rep, k, want_proba=True, views_per_point=G)
        assert np.array_equal(bits(pr)[exact], bits(proba)[exact])
        assert np.array_equal(bits(pr[:, 1]), bits(pr[:, 3]))
        want_i, want_s, want_m = vc.mean_topk(np.repeat(proba, G, axis=0), G, k)
        assert np.array_equal(idx, want_i) and np.array_equal(bits(sc), bits(want_s)) and np.array_equal(bits(pr), bits(want_m))
        if G == 2:
            assert np.array_equal(idx, ti) and np.array_equal(bits(sc), bits(ts)) and np.array_equal(bits(pr), bits(proba))
    head.close()


@pytest.mark.parametrize("name", ["head_fixture", "head108"])
def test_one_nan_view_leaves_the_other_points_alone(name):
    head = _load(name)._head
    K = head.n_classes
    G, P = 3, 6
    X = np.load(GOLDEN / f"{name}_io.npz")["X"][:P * G].copy()
    bad = X.copy()
    bad[2 * G + 1] = np.nan                                              # the middle view of point 2
    keep = np.arange(P) != 2
    for k in (1, 3, K):
        ci, cs = head.topk(X, k, views_per_point=G)
        idx, sc = head.topk(bad, k, views_per_point=G)
        assert len(set(idx[2].tolist())) == k and idx[2].min() >= 0 and idx[2].max() < K
        assert np.array_equal(idx[keep], ci[keep]) and np.array_equal(bits(sc[keep]), bits(cs[keep]))


# ---- 8. a chunk edge that would split a point ----

def test_the_row_chunk_never_splits_a_point():
    """21 900 points x 3 views = 65 700 rows, tiled on the device from 100 points: 65 536 % 3 == 1, so a chunk of 65 536 rows
    would end inside point 21 845."""
    import torch
    head = _load("head108")._head
    G, k, period, P = 3, 3, 100, 21900
    assert 65536 % G == 1 and P * G > 65536 and P % period == 0
    X = np.load(GOLDEN / "head108_io.npz")["X"]
    rng = np.random.default_rng(3)
    base = np.ascontiguousarray(X[rng.integers(0, len(X), period * G)])  # 300 rows: 100 points of 3 unrelated views
    xd = torch.from_numpy(base).cuda().repeat(P // period, 1).contiguous()
    assert xd.shape[0] == P * G
    idx, sc = head.topk(xd, k, views_per_point=G)
    first_i, first_s = head.topk(xd[:period * G], k, views_per_point=G)
    torch.cuda.synchronize()
    idx, sc, first_i, first_s = (t.cpu().numpy() for t in (idx, sc, first_i, first_s))
    assert idx.shape == (P, k)
    assert np.array_equal(idx, np.tile(first_i, (P // period, 1)))
    assert np.array_equal(bits(sc), np.tile(bits(first_s), (P // period, 1)))
    lo = 21845 - 100                                                     # 200 points around the edge
    proba, _ = head.predict(xd[lo * G:(lo + 200) * G])
    want_i, want_s, _ = vc.mean_topk(proba.cpu().numpy(), G, k)
    assert np.array_equal(idx[lo:lo + 200], want_i) and np.array_equal(bits(sc[lo:lo + 200]), bits(want_s))


# ---- 9. patches -> backbone -> mean -> top-k ----

@pytest.fixture(scope="module")
def backbone(checkpoint_path):
    from mermaid_classifier_amd.backbone import Backbone
    bb = Backbone(str(checkpoint_path), device=0, max_batch=16)
    yield bb
    bb.close()


def test_classify_patches_views_is_extract_then_topk_views(backbone):
    import torch
    from mermaid_classifier_amd import PointClassifier
    from oracle import efficientnet_b0_ref as ref
    pred = _load("head108")
    pc = PointClassifier(backbone, pred)
    five = ref.natural_patches(5, seed=21)
    k, G = 3, 4
    patches = np.ascontiguousarray(np.tile(five, (G, 1, 1, 1)))          # 20 patches = 5 points x 4 views, every point another mix
    feats = backbone.extract(patches)
    want_i, want_s = pred._head.topk(feats, k, views_per_point=G)
    got = pc.classify_patches(patches, k, views_per_point=G)
    assert got.indices.shape == (5, k) and got.rowcols is None
    assert np.array_equal(got.indices, want_i) and np.array_equal(got.scores, want_s.astype(np.float64))
    dev = pc.classify_patches(torch.from_numpy(patches).cuda(), k, views_per_point=G)
    assert np.array_equal(dev.indices, want_i) and np.array_equal(dev.scores, want_s.astype(np.float64))
    # 1366 points x 3 views = 4098 patches: 4096 % 3 == 1, a chunk of 4096 patches would end inside point 1365
    G, P = 3, 1366
    tiled = torch.from_numpy(five).cuda().repeat(-(-P * G // 5), 1, 1, 1)[:P * G].contiguous()
    di, ds = pc.topk_device(tiled, k, views_per_point=G)
    torch.cuda.synchronize()
    di, ds = di.cpu().numpy(), ds.cpu().numpy()
    assert di.shape == (P, k)
    # patch i is five[i % 5], so point p holds the patches of point p % 5
    reps = -(-P // 5)
    assert np.array_equal(di, np.tile(di[:5], (reps, 1))[:P]) and np.array_equal(bits(ds), np.tile(bits(ds[:5]), (reps, 1))[:P])
    f5 = backbone.extract(np.ascontiguousarray(np.tile(five, (G, 1, 1, 1))))
    wi, ws = pred._head.topk(f5, k, views_per_point=G)
    assert np.array_equal(di[:5], wi) and np.array_equal(bits(ds[:5]), bits(ws))


def test_classify_patches_views_with_one_view_per_point_is_mmc_classify_patches(backbone):
    """mmc_classify_patches_views with G = 1 through the C ABI (the Python front-ends send one view per point to
    mmc_classify_patches), host and device arguments: the bits of mmc_classify_patches."""
    import torch
    from mermaid_classifier_amd import _lib
    from oracle import efficientnet_b0_ref as ref
    lib = _lib.lib()
    pred = _load("head108")
    patches = ref.natural_patches(6, seed=33)
    n, k = len(patches), 3
    stream = int(torch.cuda.current_stream(0).cuda_stream)
    flags = _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST
    out = {e: (np.full((n, k), -1, np.int32), np.full((n, k), -1, np.float32)) for e in ("plain", "views")}
    _lib.check(lib.mmc_classify_patches(backbone._h, pred._head._h, patches.ctypes.data, n, k, out["plain"][0].ctypes.data,
                                        out["plain"][1].ctypes.data, flags, stream))
    _lib.check(lib.mmc_classify_patches_views(backbone._h, pred._head._h, patches.ctypes.data, n, 1, k, out["views"][0].ctypes.data,
                                              out["views"][1].ctypes.data, flags, stream))
    assert np.array_equal(out["views"][0], out["plain"][0]) and np.array_equal(bits(out["views"][1]), bits(out["plain"][1]))
    assert out["plain"][0].min() >= 0
    pd = torch.from_numpy(patches).cuda()
    di = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
    ds = torch.full((n, k), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.mmc_classify_patches_views(backbone._h, pred._head._h, pd.data_ptr(), n, 1, k, di.data_ptr(), ds.data_ptr(), 0, stream))
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy(), out["plain"][0]) and np.array_equal(bits(ds.cpu().numpy()), bits(out["plain"][1]))


# ---- 10. images -> labels with views ----

def test_point_classifier_with_views_is_the_composed_route(backbone, images):
    """batch_patches = 10 with 4 views: the capacity becomes 8 patches = 2 points, so the first image's 5 points span three
    passes and the second image starts inside the third.  Composed route: view_patch -> Backbone.extract -> the predict rows ->
    mean_topk, compared with the bitwise standard of test_classify_images_is_bitwise_the_composed_route."""
    from mermaid_classifier_amd import PointClassifier
    pred = _load("head108")
    views = (0, 1, 6, 9)
    rowcols = [[(0, 0), (228, 240), (114, 120), (3, 237), (200, 17)], [(0, 599), (320, 300), (639, 0)]]
    k = 3
    pc = PointClassifier(backbone, pred, batch_patches=10, views=views)
    got = pc.classify_images(images, rowcols, k)
    assert [len(g) for g in got] == [5, 3]
    for g, im, rc in zip(got, images, rowcols):
        feats = backbone.extract(vc.view_patches(im, rc, views))
        proba, _ = pred._head.predict(feats)
        want_i, want_s, _ = vc.mean_topk(proba, len(views), k)
        assert g.rowcols == rc and g.indices.shape == (len(rc), k)
        assert np.array_equal(g.indices, want_i) and np.array_equal(g.scores, want_s.astype(np.float64))
        assert g.labels == [[pred.classes[j] for j in row] for row in want_i.tolist()]
    one = pc.classify_image(images[1], rowcols[1], k)
    assert np.array_equal(one.indices, got[1].indices) and np.array_equal(one.scores, got[1].scores)
    # views=(0,) is the classifier of before
    plain = PointClassifier(backbone, pred, batch_patches=10).classify_images(images, rowcols, k)
    zero = PointClassifier(backbone, pred, batch_patches=10, views=(0,)).classify_images(images, rowcols, k)
    for a, b, im, rc in zip(plain, zero, images, rowcols):
        assert np.array_equal(a.indices, b.indices) and np.array_equal(a.scores, b.scores)
        proba, _ = pred._head.predict(backbone.extract(vc.view_patches(im, rc, (0,))))
        want_i, want_s, _ = vc.mean_topk(proba, 1, k)
        assert np.array_equal(b.indices, want_i) and np.array_equal(b.scores, want_s.astype(np.float64))


# ---- 11. images -> features with views ----

def test_extract_images_with_views_is_point_major(backbone, images):
    from mermaid_classifier_amd import crop_patches_device
    from mermaid_classifier_amd.pipeline import BatchedExtractor
    views = (0, 3, 12)
    rowcols = [[(0, 0), (228, 240), (114, 120), (3, 237), (200, 17)], [], [(0, 599), (320, 300)]]
    ims = [images[0], images[0], images[1]]
    ex = BatchedExtractor(backbone, batch_patches=7)                     # capacity 6 = 2 points: the first image spans passes
    got = ex.extract_images(ims, rowcols, views=views)
    assert [g.shape for g in got] == [(15, backbone.feature_dim), (0, backbone.feature_dim), (6, backbone.feature_dim)]
    for g, im, rc in zip(got, ims, rowcols):
        if rc:
            want = backbone.extract(vc.view_patches(im, rc, views))      # row p*3 + g = view views[g] of point p
            assert np.array_equal(bits(g), bits(want))
            cut = crop_patches_device(im, rc, views=views).cpu().numpy()
            assert np.array_equal(cut, vc.view_patches(im, rc, views))
    plain = ex.extract_images(ims, rowcols)
    zero = ex.extract_images(ims, rowcols, views=(0,))
    for a, b, im, rc in zip(plain, zero, ims, rowcols):
        assert a.shape == (len(rc), backbone.feature_dim) and np.array_equal(bits(a), bits(b))
        if rc:
            assert np.array_equal(bits(a), bits(backbone.extract(vc.view_patches(im, rc, (0,)))))
    assert np.array_equal(crop_patches_device(ims[0], rowcols[0]).cpu().numpy(), vc.view_patches(ims[0], rowcols[0], (0,)))
