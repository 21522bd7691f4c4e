"""Cross-image batching front-end: many images' points -> one stream of large GPU batches.

The reference walks images one at a time (scripts/build_feature_bucket.py:749-786): load, whole-image
reflect pad on the CPU, per-patch PIL crops, ToTensor/Normalize, forward at batch 10, ``.tolist()``.
Here an image is uploaded once, its patches are cut by ``mmc_crop_patches`` (index arithmetic, no padded
copy) straight into a device buffer shared by consecutive images, and the backbone runs whenever
``batch_patches`` patches are resident -- so small point counts per image (10-25 in the reference's
data) still produce full 256-patch passes.  Output order and grouping are the reference's: one
``(n_points, 1280)`` float32 array per image, rows in ``rowcols`` order, or ``ImageFeatures`` objects with
``get_array((row, col))`` (mermaid_classifier/pyspacer/annotation.py:250).
"""

from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .backbone import Backbone, PATCH, _current_stream_ptr, check_views
from .spacer_shim import ImageFeatures, PointFeatures


def check_extract_inputs(image: np.ndarray, rowcols: Sequence[Tuple[int, int]], name: str = "image") -> None:
    """pyspacer ``check_extract_inputs`` as the reference calls it (annotation.py:240): every point must lie
    inside the image; raises ValueError naming the offending point."""
    h, w = image.shape[:2]
    for r, c in rowcols:
        if not (0 <= int(r) < h and 0 <= int(c) < w):
            raise ValueError(f"{name}: point ({r}, {c}) is outside the {h}x{w} image")
    if h <= PATCH or w <= PATCH:
        raise ValueError(f"{name}: image {h}x{w} must exceed the {PATCH}-pixel crop in both dimensions")


def prepare_image(idx: int, image, rowcols) -> Tuple[np.ndarray, np.ndarray]:
    """One image and its points as the front-ends take them: grayscale promoted to RGB, contiguous uint8 (H,W,3), points as
    (n,2) int32, every point checked against the image (``check_extract_inputs``).  Host work only."""
    im = np.asarray(image)
    if im.ndim == 2:
        im = np.stack([im] * 3, axis=-1)
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] < 3:
        raise ValueError(f"image {idx}: expected uint8 (H,W,3); got {im.dtype} {im.shape}")
    im = np.ascontiguousarray(im[..., :3])
    rc = np.ascontiguousarray(np.asarray(list(rowcols), dtype=np.int32).reshape(-1, 2))
    if len(rc):
        check_extract_inputs(im, rc, name=f"image {idx}")
    return im, rc


class PatchBatcher:
    """The buffer / flush machinery of the cross-image front-ends (``BatchedExtractor``: features, ``classify.PointClassifier``:
    top-k labels): two device patch buffers filled by ``mmc_crop_patches`` on a copy stream, one pass per full buffer on the
    compute stream, the previous pass's results collected from pinned memory while the next one runs.  A subclass says what a
    pass is: ``_launch(slot, patches, fill, ctx)`` enqueues the work on the current stream, ``_download(slot, fill, ctx)`` the copy of
    its results into pinned memory, ``_fetch(slot, count, ctx)`` returns them (a tuple of host arrays with ``count`` rows each) once
    the pass is done.

    With ``views`` (``backbone.check_views``) other than ``(0,)`` every point is cut G = len(views) times, point-major, by
    ``mmc_crop_patches_views``; a point's G patches never straddle a pass (for the run the buffer capacity is rounded down to a
    multiple of G).  ``fill`` counts patches; ``_download`` / ``_fetch`` count result rows: G per point, or one per point for a
    subclass with ``mean_over_views`` (its pass averages a point's views)."""

    mean_over_views = False

    def __init__(self, backbone: Backbone, batch_patches: int = 1024):
        import torch
        self.bb = backbone
        self.cap = int(batch_patches)
        if self.cap < 1:
            raise ValueError(f"batch_patches must be >= 1; got {batch_patches}")
        self.dev = torch.device("cuda", backbone.device_index)
        # two patch buffers: while the backbone works through one, the next images are cut / uploaded into the other on a
        # separate copy stream (a buffer is refilled only after the pass that read it has finished: per-buffer event)
        self._bufs = [torch.empty((self.cap, PATCH, PATCH, 3), dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self._free = [torch.cuda.Event(), torch.cuda.Event()]
        self._done = [torch.cuda.Event(), torch.cuda.Event()]
        self._copy_stream = torch.cuda.Stream(device=self.dev)
        self._buf = self._bufs[0]

    def _crop_into(self, image: np.ndarray, rowcols: np.ndarray, offset: int) -> None:
        n = rowcols.shape[0]
        dst = self._buf[offset:offset + n]
        _lib.check(_lib.lib().mmc_crop_patches(image.ctypes.data, image.shape[0], image.shape[1], rowcols.ctypes.data, n,
                                               dst.data_ptr(), _lib.MMC_IN_HOST, self.bb.device_index,
                                               int(self._copy_stream.cuda_stream)))

    def _crop_views_into(self, image: np.ndarray, rowcols: np.ndarray, views: Tuple[int, ...], offset: int) -> None:
        g = len(views)
        rc = np.ascontiguousarray(np.repeat(rowcols, g, axis=0))
        codes = np.ascontiguousarray(np.tile(np.asarray(views, np.uint8), rowcols.shape[0]))
        n = rc.shape[0]
        dst = self._buf[offset:offset + n]
        _lib.check(_lib.lib().mmc_crop_patches_views(image.ctypes.data, image.shape[0], image.shape[1], rc.ctypes.data, n,
                                                     codes.ctypes.data, dst.data_ptr(), _lib.MMC_IN_HOST, self.bb.device_index,
                                                     int(self._copy_stream.cuda_stream)))

    def _launch(self, slot: int, patches, fill: int, ctx) -> None:
        raise NotImplementedError

    def _download(self, slot: int, fill: int, ctx) -> None:
        raise NotImplementedError

    def _fetch(self, slot: int, count: int, ctx) -> tuple:
        raise NotImplementedError

    def _run(self, images: Iterable[np.ndarray], rowcols_per_image: Iterable[Sequence[Tuple[int, int]]], ctx=None,
             views: Tuple[int, ...] = (0,)):
        """-> (per image: a tuple of arrays, one per result kind, rows in ``rowcols`` order; None for an image without points,
        the checked (n, 2) int32 points per image)."""
        import torch
        plain = tuple(views) == (0,)                # today's path: mmc_crop_patches, one patch and one result row per point
        g = len(views)
        if self.cap < g:
            raise ValueError(f"batch_patches = {self.cap} cannot hold the {g} views of one point")
        cap = self.cap // g * g                     # patches per pass: whole points only
        rpp = 1 if self.mean_over_views else g      # result rows per point
        out: List[Optional[tuple]] = []
        points: List[np.ndarray] = []
        pending: List[Tuple[int, int, int]] = []   # (image index, offset in buffer, n)
        fill = 0
        cur = 0                                     # buffer being filled
        in_flight = None                            # (slot, count, pending list) of the pass launched last
        compute = torch.cuda.current_stream(self.dev)
        self._buf = self._bufs[cur]
        self._copy_stream.wait_stream(compute)      # whatever wrote these buffers before is done before the first cut lands

        def collect(job):
            slot, count, items = job
            self._done[slot].synchronize()                       # this pass's D2H only -- not whatever was enqueued after it
            res = self._fetch(slot, count, ctx)
            for idx, off, n in items:
                part = tuple(a[off:off + n] for a in res)
                out[idx] = part if out[idx] is None else tuple(np.concatenate([o, q]) for o, q in zip(out[idx], part))

        def flush():
            nonlocal fill, pending, cur, in_flight
            if fill == 0:
                return
            compute.wait_stream(self._copy_stream)              # the cuts of this buffer have landed
            self._launch(cur, self._bufs[cur][:fill], fill, ctx)   # asynchronous on the compute stream
            self._free[cur].record(compute)
            self._download(cur, fill // g * rpp, ctx)            # pinned: the D2H is stream-ordered too
            self._done[cur].record(compute)
            job = (cur, fill // g * rpp, pending)
            if in_flight is not None:
                collect(in_flight)                               # the previous pass; this one keeps running meanwhile
            in_flight = job
            fill, pending = 0, []
            cur ^= 1
            self._buf = self._bufs[cur]
            self._copy_stream.wait_event(self._free[cur])        # refill only after the pass that read this buffer

        for idx, (image, rowcols) in enumerate(zip(images, rowcols_per_image)):
            im, rc = prepare_image(idx, image, rowcols)
            out.append(None)
            points.append(rc)
            start = 0
            while start < len(rc):                      # an image with more points than the buffer spans flushes
                take = min(len(rc) - start, (cap - fill) // g)             # points
                if take == 0:
                    flush()
                    continue
                if plain:
                    self._crop_into(im, rc[start:start + take], fill)
                else:
                    self._crop_views_into(im, rc[start:start + take], views, fill)
                pending.append((idx, fill // g * rpp, take * rpp))
                fill += take * g
                start += take
        flush()
        if in_flight is not None:
            collect(in_flight)
        return out, points


class BatchedExtractor(PatchBatcher):
    """Feeds a ``Backbone`` with cross-image batches.  ``batch_patches`` bounds the device patch buffer."""

    def __init__(self, backbone: Backbone, batch_patches: int = 1024):
        import torch
        super().__init__(backbone, batch_patches)
        self._host = [torch.empty((self.cap, backbone.feature_dim), dtype=torch.float32).pin_memory() for _ in range(2)]
        # one device feature buffer per slot: a pass sees the same (patches, features) pair every time its slot comes round, so the
        # library's HIP-graph cache keeps hitting (a fresh output tensor per flush would mint a new combination per pass)
        self._fdev = [torch.empty((self.cap, backbone.feature_dim), dtype=torch.float32, device=self.dev) for _ in range(2)]

    def _launch(self, slot, patches, fill, ctx):
        self.bb.extract(patches, out=self._fdev[slot][:fill])

    def _download(self, slot, fill, ctx):
        self._host[slot][:fill].copy_(self._fdev[slot][:fill], non_blocking=True)

    def _fetch(self, slot, count, ctx):
        return (self._host[slot][:count].numpy().copy(),)

    def extract_images(self, images: Iterable[np.ndarray], rowcols_per_image: Iterable[Sequence[Tuple[int, int]]],
                       views: Sequence[int] = (0,)) -> List[np.ndarray]:
        """-> one (n_points * G, 1280) float32 array per image (empty arrays for images without points), G = len(views): row
        ``p*G + g`` is view ``views[g]`` (``backbone.check_views``) of point ``p``.  ``views=(0,)`` is one row per point, through the
        calls and with the bits of before views existed.  ``batch_patches < G`` is a ValueError."""
        vw = check_views(views)
        out, _ = self._run(images, rowcols_per_image, views=vw)
        return [o[0] if o is not None else np.zeros((0, self.bb.feature_dim), np.float32) for o in out]

    def extract_image_features(self, images, rowcols_per_image) -> List[ImageFeatures]:
        rowcols_per_image = [list(rc) for rc in rowcols_per_image]
        feats = self.extract_images(images, rowcols_per_image)
        res = []
        for f, rc in zip(feats, rowcols_per_image):
            pfs = [PointFeatures(int(r), int(c), row.tolist()) for (r, c), row in zip(rc, f)]
            res.append(ImageFeatures(pfs, True, self.bb.feature_dim, len(pfs)))
        return res
