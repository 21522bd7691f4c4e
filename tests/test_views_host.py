"""CPU tests of patch views (include/mmc.h, "patch views"): the ABI surface, the argument checks that fire without a device, the
Python checks that fire before one is touched, and the numpy checker of tests/views_checker.py on a hand-written image."""

import re
from pathlib import Path

import numpy as np
import pytest

import views_checker as vc
from mermaid_classifier_amd import ALL_ORIENTATIONS, check_views          # the feature under test: absent, nothing here runs

ROOT = Path(__file__).resolve().parent.parent
NEW = ("mmc_crop_patches_views", "mmc_head_topk_views", "mmc_classify_patches_views")


def test_library_exports_the_view_entry_points_as_the_header_declares_them():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    header = (ROOT / "include" / "mmc.h").read_text()
    for sym in NEW:
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
        decl = re.search(r"\bint " + sym + r"\(([^;]*)\);", header).group(1)
        n_args = len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(","))
        assert len(getattr(lib, sym).argtypes) == n_args, sym
    assert int(re.search(r"#define MMC_VIEWS_MAX (\d+)", header).group(1)) == 16 == _lib.MMC_VIEWS_MAX


def test_null_arguments_are_argument_errors_with_a_message():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    assert lib.mmc_crop_patches_views(None, 300, 300, None, 1, None, None, _lib.MMC_IN_HOST, 0, None) == _lib.MMC_ERR_ARG
    assert b"NULL argument" in lib.mmc_last_error()
    assert lib.mmc_head_topk_views(None, None, 1, 1, 1, None, None, None, 0, None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error()
    assert lib.mmc_classify_patches_views(None, None, None, 1, 1, 1, None, None, 0, None) == _lib.MMC_ERR_ARG
    assert b"backbone handle is NULL" in lib.mmc_last_error()


def test_bad_group_sizes_k_and_host_view_codes_need_no_device():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    for G in (0, 17, -1):
        assert lib.mmc_head_topk_views(None, None, 1, G, 1, None, None, None, 0, None) == _lib.MMC_ERR_ARG
        assert f"G = {G} views per point is outside [1, 16]".encode() in lib.mmc_last_error()
        assert lib.mmc_classify_patches_views(None, None, None, 1, G, 1, None, None, 0, None) == _lib.MMC_ERR_ARG
        assert f"G = {G} views per point is outside [1, 16]".encode() in lib.mmc_last_error()
    assert lib.mmc_head_topk_views(None, None, 1, 2, 0, None, None, None, 0, None) == _lib.MMC_ERR_ARG
    assert b"k = 0" in lib.mmc_last_error()
    assert lib.mmc_classify_patches_views(None, None, None, 1, 2, 0, None, None, 0, None) == _lib.MMC_ERR_ARG
    assert b"k = 0" in lib.mmc_last_error()
    image = np.zeros((300, 300, 3), np.uint8)
    rc = np.array([[10, 10], [20, 20], [30, 30]], np.int32)
    codes = np.array([0, 15, 16], np.uint8)
    out = np.zeros(8, np.uint8)                                    # never written: the call fails on the third code
    assert lib.mmc_crop_patches_views(image.ctypes.data, 300, 300, rc.ctypes.data, 3, codes.ctypes.data, out.ctypes.data,
                                      _lib.MMC_IN_HOST, 0, None) == _lib.MMC_ERR_ARG
    assert b"view code 16 of patch 2" in lib.mmc_last_error()
    assert lib.mmc_crop_patches_views(image.ctypes.data, 224, 300, rc.ctypes.data, 3, codes.ctypes.data, out.ctypes.data,
                                      _lib.MMC_IN_HOST, 0, None) == _lib.MMC_ERR_ARG
    assert b"must exceed the crop size" in lib.mmc_last_error()    # the one-reflection condition is still checked


# ---- the Python checks: every ValueError before the device ----

class _NoDevice:
    """Stands where a device handle would: any use of it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name})")


class _Backbone:
    feature_dim = 8
    device_index = 0
    _h = _NoDevice()


def _predictor(k_classes=4, input_dim=8):
    from mermaid_classifier_amd.inference import Predictor
    return Predictor(_NoDevice(), [f"c{i}" for i in range(k_classes)], input_dim)


BAD_VIEWS = [(), [], (16,), (0, -1), (0.5,), (True,), tuple(range(16)) + (0,), 3, None, ("0",)]


def test_check_views_and_the_package_exports():
    import mermaid_classifier_amd as m
    assert "check_views" in m.__all__ and "ALL_ORIENTATIONS" in m.__all__ and m.ALL_ORIENTATIONS == tuple(range(8))
    assert m.check_views([0, np.int64(9), 15]) == (0, 9, 15)
    assert m.check_views(tuple(range(16))) == tuple(range(16))
    assert m.check_views((3, 3)) == (3, 3)                          # repeats are the caller's business
    for bad in BAD_VIEWS:
        with pytest.raises(ValueError, match="view"):
            m.check_views(bad)


def test_view_argument_errors_come_before_the_device():
    from mermaid_classifier_amd import PointClassifier, crop_patches_device
    from mermaid_classifier_amd.inference import DeviceHead
    from mermaid_classifier_amd.pipeline import BatchedExtractor
    image = np.zeros((300, 400, 3), np.uint8)
    for bad in BAD_VIEWS:
        with pytest.raises(ValueError, match="view"):
            PointClassifier(_Backbone(), _predictor(), batch_patches=64, views=bad)
        with pytest.raises(ValueError, match="view"):
            crop_patches_device(image, [(5, 5)], device=_NoDevice(), views=bad)
        with pytest.raises(ValueError, match="view"):
            BatchedExtractor.extract_images(_NoDevice(), [image], [[(5, 5)]], views=bad)
    with pytest.raises(ValueError, match="batch_patches = 3 cannot hold the 4 views"):
        PointClassifier(_Backbone(), _predictor(), batch_patches=3, views=(0, 1, 2, 3))
    small = BatchedExtractor.__new__(BatchedExtractor)             # no device buffers: only the capacity is looked at
    small.cap = 2
    small.bb = _NoDevice()
    with pytest.raises(ValueError, match="batch_patches = 2 cannot hold the 3 views"):
        small.extract_images([image], [[(5, 5)]], views=(0, 3, 12))
    pc = PointClassifier(_Backbone(), _predictor(), batch_patches=8, views=(0, 1, 6, 9))
    assert pc.views == (0, 1, 6, 9)
    with pytest.raises(ValueError, match=r"point \(300, 1\) is outside"):          # the point checks still come first
        pc.classify_image(image, [(10, 10), (300, 1)])
    patches = np.zeros((6, 224, 224, 3), np.uint8)
    with pytest.raises(ValueError, match="6 rows are not a whole number of points at views_per_point = 4"):
        pc.classify_patches(patches, k=1, views_per_point=4)
    for bad in (0, 17, 1.5, True, None):
        with pytest.raises(ValueError, match="views_per_point must be"):
            pc.classify_patches(patches, k=1, views_per_point=bad)
        with pytest.raises(ValueError, match="views_per_point must be"):
            _predictor().predict_topk(np.zeros((6, 8), np.float32), k=1, views_per_point=bad)
    pred = _predictor()
    with pytest.raises(ValueError, match="6 rows are not a whole number of points at views_per_point = 4"):
        pred.predict_topk(np.zeros((6, 8), np.float32), k=2, views_per_point=4)
    with pytest.raises(ValueError, match="k must be"):
        pred.predict_topk(np.zeros((6, 8), np.float32), k=0, views_per_point=3)
    labels, scores = pred.predict_topk(np.zeros((0, 8), np.float32), k=2, views_per_point=3)       # the empty batch
    assert labels == [] and scores.shape == (0, 2)
    head = DeviceHead.__new__(DeviceHead)                          # the wrapper's own checks, without a handle
    head._h, head.input_dim, head.n_classes, head.device_index = _NoDevice(), 8, 4, 0
    with pytest.raises(ValueError, match="not a whole number of points"):
        head.topk(np.zeros((7, 8), np.float32), 2, views_per_point=2)
    head._h = None                                                 # (so that __del__ has nothing to close)


# ---- the checker itself ----

def _ramp(h=300, w=310):
    """image[y, x] = (y, x, y + 2x) mod 251: every pixel of a 224-window differs from its mirror images."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([y % 251, x % 251, (y + 2 * x) % 251], axis=-1).astype(np.uint8)


def test_views_0_to_7_are_the_orbit_of_view_0():
    im = _ramp()
    assert check_views(ALL_ORIENTATIONS) == tuple(range(8))
    p = [vc.view_patch(im, 150, 160, v) for v in ALL_ORIENTATIONS]
    for a in range(8):
        assert p[a].shape == (224, 224, 3) and p[a].dtype == np.uint8 and p[a].flags.c_contiguous
        for b in range(a + 1, 8):
            assert not np.array_equal(p[a], p[b]), (a, b)
    from oracle import pyspacer_ref
    assert np.array_equal(p[0], pyspacer_ref.crop_patches(im, [(150, 160)])[0])
    # the group generated by rot90 and fliplr, walked from view 0: r quarter turns of the (flipped) patch
    for r in range(4):
        assert np.array_equal(p[r], np.rot90(p[0], r))
        assert np.array_equal(p[4 + r], np.rot90(np.fliplr(p[0]), r))
        assert np.array_equal(p[(r + 1) % 4], np.rot90(p[r]))                       # closed under a further quarter turn
        assert np.array_equal(p[4 + (r + 1) % 4], np.rot90(p[4 + r]))
    assert np.array_equal(np.fliplr(p[1]), p[7]) and np.array_equal(np.fliplr(p[4]), p[0])      # and under a further flip
    # views 8..15 are the same orbit of view 8
    q = [vc.view_patch(im, 150, 160, 8 + v) for v in range(8)]
    for r in range(4):
        assert np.array_equal(q[r], np.rot90(q[0], r)) and np.array_equal(q[4 + r], np.rot90(np.fliplr(q[0]), r))
    # a transposing view at hand-computed positions: view 1 = rot90 (counterclockwise): out[i, j] = B[j, 223 - i]
    assert tuple(p[1][0, 0]) == tuple(p[0][0, 223]) and tuple(p[1][223, 0]) == tuple(p[0][0, 0])
    assert tuple(p[1][10, 200]) == tuple(p[0][200, 213])
    # view 6 = rot90(fliplr(B), 2) = flipud(B)
    assert np.array_equal(p[6], p[0][::-1])


def test_context_view_is_the_rounded_mean_of_four_pixels():
    im = _ramp(500, 520)
    row, col = 250, 260                                            # interior: the window is rows 26..473, columns 36..483
    b = vc.view_patch(im, row, col, 8)
    for y, x in ((0, 0), (17, 100), (223, 39)):                    # window rows 2y, 2y + 1 = image rows row - 224 + 2y (+ 1)
        r0, c0 = row - 224 + 2 * y, col - 224 + 2 * x
        assert 0 <= r0 and r0 + 1 < im.shape[0] and 0 <= c0 and c0 + 1 < im.shape[1]
        four = im[r0:r0 + 2, c0:c0 + 2].astype(np.int64).reshape(4, 3)
        want = [(int(four[:, c].sum()) + 2) // 4 for c in range(3)]
        assert b[y, x].tolist() == want, (y, x)
    # rounding is half up: four pixels 1, 2, 2, 1 -> (6 + 2) >> 2 = 2, and 0, 0, 1, 0 -> 0, 1, 1, 0 -> 1
    flat = np.zeros((500, 500, 3), np.uint8)
    flat[250:252, 250:252, 0] = [[1, 2], [2, 1]]
    flat[250:252, 250:252, 1] = [[0, 0], [1, 0]]
    flat[250:252, 250:252, 2] = [[0, 1], [1, 0]]
    assert vc.view_patch(flat, 250, 250, 8)[112, 112].tolist() == [2, 0, 1]


def test_corner_points_reflect_as_the_indexed_crop_does():
    from oracle import pyspacer_ref
    im = _ramp(229, 241)
    for row, col in ((0, 0), (0, 240), (228, 0), (228, 240)):
        assert np.array_equal(vc.view_patch(im, row, col, 0), pyspacer_ref.crop_patches_indexed(im, [(row, col)], 224)[0])
        w = pyspacer_ref.crop_patches_indexed(im, [(row, col)], 448)[0].astype(np.int32)
        want = ((w[0::2, 0::2] + w[0::2, 1::2] + w[1::2, 0::2] + w[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        assert np.array_equal(vc.view_patch(im, row, col, 8), want)
        assert np.array_equal(vc.view_patch(im, row, col, 13), np.rot90(want[:, ::-1], 1))


def test_mean_topk_sums_left_to_right_in_fp32_and_sorts_stably():
    # (a + b) + c != a + (b + c) in fp32 for these three: the checker must give the left-to-right value
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    rows = np.array([[a, 0.5, 0.5], [b, 0.25, 0.25], [c, 0.25, 0.25]], np.float32)
    idx, sc, mean = vc.mean_topk(rows, 3, 3)
    assert mean[0, 0] == np.float32(np.float32(np.float32(a + b) + c) / np.float32(3)) and np.float32(a + b) == a
    assert idx.tolist() == [[0, 1, 2]] and idx.dtype == np.int32 and sc.dtype == np.float32       # the tie 1, 2 in class order
    one = np.array([[0.2, 0.5, 0.3], [0.6, 0.1, 0.3]], np.float32)
    idx, sc, mean = vc.mean_topk(one, 1, 2)                        # G = 1: the rows themselves
    assert np.array_equal(mean.view(np.uint32), one.view(np.uint32)) and idx.tolist() == [[1, 2], [0, 2]]
    assert vc.view_patches(_ramp(), [(100, 100), (150, 120)], (0, 5)).shape == (4, 224, 224, 3)
