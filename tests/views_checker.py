"""What tests/test_views_host.py and tests/test_gpu_views.py share: a numpy evaluation of the view definition of include/mmc.h
("patch views": that text is the definition, this module follows it line by line) and of the view-averaged top-k.  Not a test
module."""

import numpy as np

from oracle import pyspacer_ref


def base_patch(image, row, col, z):
    """The base patch B of a point: the reference's own crop (whole-image reflect pad + slice), 224 or 448 pixels wide."""
    if not z:
        return pyspacer_ref.crop_patches(image, [(row, col)], 224)[0]
    w = pyspacer_ref.crop_patches(image, [(row, col)], 448)[0].astype(np.int32)
    return ((w[0::2, 0::2] + w[0::2, 1::2] + w[1::2, 0::2] + w[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def view_patch(image, row, col, v):
    """View ``v`` of the point (row, col): (224, 224, 3) uint8, contiguous."""
    r, f, z = v & 3, (v >> 2) & 1, (v >> 3) & 1
    b = base_patch(image, row, col, z)
    return np.ascontiguousarray(np.rot90(b[:, ::-1] if f else b, k=r, axes=(0, 1)))


def view_patches(image, rowcols, views):
    """Point-major: patch p * G + g is view views[g] of point p."""
    return np.stack([view_patch(image, r, c, v) for r, c in rowcols for v in views])


def mean_topk(proba_rows, G, k):
    """proba_rows: (P * G, K) float32, rows p G .. p G + G - 1 the views of point p -> (idx (P, k) int32, scores (P, k) float32,
    mean (P, K) float32): a left-to-right fp32 sum over the views, / float32(G), then the stable descending sort of
    tests/test_gpu_classify.py's host_topk (equal scores stay in class order)."""
    p = np.asarray(proba_rows, np.float32)
    p = p.reshape(-1, G, p.shape[1])
    acc = p[:, 0].copy()
    for g in range(1, G):
        acc = acc + p[:, g]
    mean = acc / np.float32(G)
    assert mean.dtype == np.float32
    order = np.argsort(-mean, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(mean, order, 1), mean
