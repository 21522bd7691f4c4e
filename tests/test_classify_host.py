"""CPU tests of on-device classification (top-k labels per point): the ABI surface, the argument checks that must fire
before a device is touched, ``PointPredictions`` and the label gather of the sharded path under gloo (worlds of 2 and 3)."""

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_library_exports_the_topk_entry_points():
    from mermaid_classifier_amd import _lib
    lib = _lib.lib()
    for sym in ("mmc_head_topk", "mmc_classify_patches"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    # NULL handles are argument errors with a message, no device needed
    assert lib.mmc_head_topk(None, None, 1, 1, None, None, None, 0, None) == _lib.MMC_ERR_ARG
    assert b"head handle is NULL" in lib.mmc_last_error()
    assert lib.mmc_classify_patches(None, None, None, 1, 1, None, None, 0, None) == _lib.MMC_ERR_ARG
    assert b"backbone handle is NULL" in lib.mmc_last_error()


def test_package_exports_the_classifier():
    import mermaid_classifier_amd as m
    assert "PointClassifier" in m.__all__ and "PointPredictions" in m.__all__
    assert m.PointClassifier is not None and m.PointPredictions is not None


class _NoDevice:
    """Stands where a device handle would: any use of it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name})")


def _predictor(k_classes=4, input_dim=8):
    from mermaid_classifier_amd.inference import Predictor
    return Predictor(_NoDevice(), [f"c{i}" for i in range(k_classes)], input_dim)


class _Backbone:
    feature_dim = 8
    device_index = 0
    _h = _NoDevice()


def test_predict_topk_argument_errors_come_before_the_device():
    pred = _predictor()
    for bad_k in (0, -1, 1.5):
        with pytest.raises(ValueError, match="k must be"):
            pred.predict_topk(np.zeros((2, 8), np.float32), k=bad_k)
    with pytest.raises(ValueError, match=r"features must be \(N, 8\)"):
        pred.predict_topk(np.zeros((2, 9), np.float32), k=1)
    with pytest.raises(ValueError, match=r"features must be \(N, 8\)"):
        pred.predict_topk(np.zeros((8,), np.float32), k=1)
    # the empty batch: k clamps to the class count, as the reference's [:k] slice does
    labels, scores = pred.predict_topk(np.zeros((0, 8), np.float32), k=3)
    assert labels == [] and scores.shape == (0, 3) and scores.dtype == np.float64
    labels, scores = pred.predict_topk(np.zeros((0, 8), np.float32), k=9)
    assert labels == [] and scores.shape == (0, 4)


def test_classify_argument_errors_come_before_the_device():
    from mermaid_classifier_amd import PointClassifier
    pc = PointClassifier(_Backbone(), _predictor(), batch_patches=4)
    patches = np.zeros((2, 224, 224, 3), np.uint8)
    image = np.zeros((300, 400, 3), np.uint8)
    for bad_k in (0, -2):
        with pytest.raises(ValueError, match="k must be"):
            pc.classify_patches(patches, k=bad_k)
        with pytest.raises(ValueError, match="k must be"):
            pc.classify_image(image, [(1, 1)], k=bad_k)
    with pytest.raises(ValueError, match="patches must be uint8"):
        pc.classify_patches(np.zeros((2, 224, 223, 3), np.uint8))
    with pytest.raises(ValueError, match="patches must be uint8"):
        pc.classify_patches(np.zeros((2, 224, 224, 3), np.float32))
    with pytest.raises(TypeError):
        pc.classify_patches([patches[0]])
    with pytest.raises(ValueError, match=r"point \(300, 1\) is outside the 300x400 image"):
        pc.classify_image(image, [(10, 10), (300, 1)])
    with pytest.raises(ValueError, match="image 1"):                    # the second image's point, found before any pass runs
        pc.classify_images([image, image], [[(10, 10)], [(5, 400)]])
    with pytest.raises(ValueError, match="expected uint8"):
        pc.classify_image(image.astype(np.float32), [(10, 10)])
    with pytest.raises(ValueError, match="must exceed the 224-pixel crop"):
        pc.classify_image(np.zeros((224, 400, 3), np.uint8), [(10, 10)])
    with pytest.raises(ValueError, match="feature_dim 8 != predictor input_dim 1280"):
        PointClassifier(_Backbone(), _predictor(input_dim=1280))
    with pytest.raises(ValueError, match="batch_patches"):
        PointClassifier(_Backbone(), _predictor(), batch_patches=0)


def test_point_predictions_as_dicts_order_duplicates_and_empty():
    from mermaid_classifier_amd import PointPredictions
    classes = ["coral", "sand", "algae"]
    rowcols = [(5, 7), (1, 2), (5, 7)]                 # (5, 7) twice: the later entry wins, as a dict assignment does
    idx = np.array([[2, 0], [1, 2], [0, 1]], np.int32)
    sc = np.array([[0.6, 0.3], [0.5, 0.25], [0.7, 0.2]], np.float32)
    pp = PointPredictions(rowcols, idx, sc, classes)
    assert len(pp) == 3 and pp.indices.dtype == np.int32 and pp.scores.dtype == np.float64
    assert pp.labels == [["algae", "coral"], ["sand", "algae"], ["coral", "sand"]]
    annotations, scores = pp.as_dicts()
    assert list(annotations) == [(5, 7), (1, 2)] and list(scores) == [(5, 7), (1, 2)]        # first-seen key order
    assert annotations == {(5, 7): ["coral", "sand"], (1, 2): ["sand", "algae"]}
    assert scores == {(5, 7): [float(np.float32(0.7)), float(np.float32(0.2))], (1, 2): [0.5, 0.25]}
    # the reference's own loop (annotation.py:252-261) on the same rows gives the same two dictionaries
    proba = np.zeros((3, 3))
    np.put_along_axis(proba, idx.astype(np.int64), sc.astype(np.float64), 1)
    from operator import itemgetter
    ann_ref, sc_ref = {}, {}
    for rc, row in zip(rowcols, proba.tolist()):
        top = sorted(zip(classes, row), key=itemgetter(1), reverse=True)
        ann_ref[rc] = [label for label, _ in top[:2]]
        sc_ref[rc] = [s for _, s in top[:2]]
    assert annotations == ann_ref and scores == sc_ref
    empty = PointPredictions([], np.zeros((0, 2), np.int32), np.zeros((0, 2)), classes)        # an image without points
    assert len(empty) == 0 and empty.labels == [] and empty.as_dicts() == ({}, {})
    with pytest.raises(ValueError, match="no \\(row, col\\) keys"):
        PointPredictions(None, idx, sc, classes).as_dicts()
    with pytest.raises(ValueError, match="2 points but 3"):
        PointPredictions(rowcols[:2], idx, sc, classes)


# ---- the label gather: gather_topk / classify_sharded under gloo ----

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


K_TOP = 3


def _expected(n_total):
    """Row i's indices and scores as a function of the global row number; the scores include patterns (a NaN payload, a
    denormal, -0.0) that only survive a gather that moves bits."""
    i = np.arange(n_total, dtype=np.int64)[:, None]
    idx = ((7 * i + np.arange(K_TOP)) % 108).astype(np.int32)
    bits = (0x3F000000 - 4099 * i - 17 * np.arange(K_TOP)).astype(np.uint32)
    if n_total > 0:
        bits[0, 0] = 0x7FC01234
    if n_total > 1:
        bits[1, 1] = 0x00000001
        bits[1, 2] = 0x80000000
    return idx, bits


def _topk_worker(rank, world, port, n_total, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mermaid_classifier_amd.dist import classify_sharded, gather_topk, shard_range
        idx, bits = _expected(n_total)
        lo, hi = shard_range(n_total, rank, world)
        calls = []

        def fake_classify(block, k):
            block = np.asarray(block)
            calls.append(block.copy())
            return (torch.from_numpy(idx[block].reshape(-1, k)), torch.from_numpy(bits[block].reshape(-1, k).view(np.float32)))

        gi, gs = classify_sharded(fake_classify, np.arange(n_total), K_TOP)
        hi_, hs = gather_topk(torch.from_numpy(idx[lo:hi]), torch.from_numpy(bits[lo:hi].view(np.float32)), n_total)
        errors = []
        try:
            gather_topk(torch.from_numpy(idx[lo:hi]).long(), torch.from_numpy(bits[lo:hi].view(np.float32)), n_total)
            errors.append("int64 indices accepted")
        except ValueError:
            pass
        q.put((rank, gi.numpy(), gs.numpy().view(np.uint32), hi_.numpy(), hs.numpy().view(np.uint32), str(gi.dtype), str(gs.dtype),
               [c.tolist() for c in calls], (lo, hi), errors))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n_total", [(2, 10), (2, 7), (3, 8), (3, 10), (3, 2), (2, 1), (2, 0), (3, 0)])
def test_gather_topk_returns_indices_and_score_bits_in_global_order(world, n_total):
    """Even and ragged shards, n_total < world and n_total = 0: every rank gets the (n_total, k) indices and the score BITS of
    every row in global order, from one collective of (n_local, 2k) int32 blocks; each rank classified only its own block."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_topk_worker, args=(r, world, port, n_total, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    idx, bits = _expected(n_total)
    assert sorted(r[0] for r in results) == list(range(world))
    for rank, gi, gbits, hi_, hbits, di, ds, calls, (lo, hi), errors in results:
        assert errors == []
        assert di == "torch.int32" and ds == "torch.float32"
        assert gi.shape == (n_total, K_TOP) and gbits.shape == (n_total, K_TOP)
        np.testing.assert_array_equal(gi, idx)
        np.testing.assert_array_equal(gbits, bits)
        np.testing.assert_array_equal(hi_, idx)
        np.testing.assert_array_equal(hbits, bits)
        assert calls == [list(range(lo, hi))]           # one call, the rank's own contiguous block


def test_gather_topk_is_one_collective(monkeypatch):
    """Indices and scores share one all_gather_into_tensor of an (n_local, 2k) int32 block (world of one, gloo)."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        from mermaid_classifier_amd.dist import gather_topk
        seen = []
        real = dist.all_gather_into_tensor

        def spy(out, send, **kw):
            seen.append((tuple(send.shape), send.dtype))
            return real(out, send, **kw)

        monkeypatch.setattr(dist, "all_gather_into_tensor", spy)
        idx, bits = _expected(5)
        gi, gs = gather_topk(torch.from_numpy(idx), torch.from_numpy(bits.view(np.float32)), 5)
        assert seen == [((5, 2 * K_TOP), torch.int32)]
        np.testing.assert_array_equal(gi.numpy(), idx)
        np.testing.assert_array_equal(gs.numpy().view(np.uint32), bits)
        with pytest.raises(ValueError, match="equal"):
            gather_topk(torch.from_numpy(idx), torch.from_numpy(bits.view(np.float32))[:, :2], 5)
    finally:
        dist.destroy_process_group()
