"""Image + points -> top-k labels and calibrated scores per point, ranked on the device.

Mirrors what ``AnnotationRun.__init__`` does with a classifier (mermaid_classifier/pyspacer/annotation.py:231-262):
``extractor(image, rowcols)`` -> ``predictor.predict_proba(feature_batch)`` -> per point
``sorted(zip(labels, proba), key=itemgetter(1), reverse=True)[:predictions_per_point]`` into the ``annotations`` and ``scores``
dictionaries.  Here the features never leave the GPU: ``mmc_classify_patches`` runs backbone, head and the top-k selection on one
stream, and only the ``(n, k)`` class indices and scores are copied back.  Order and ties are the reference's (score descending,
equal scores in class order); the probabilities are those of ``Predictor.predict_proba``, bit for bit.
"""

from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .backbone import PATCH, _current_stream_ptr, check_views, check_views_per_point
from .pipeline import PatchBatcher, prepare_image


class PointPredictions:
    """The predictions for one image's points (or one patch batch): ``rowcols`` [(row, col)] (None for bare patches),
    ``indices`` (n, k) int32 class indices, ``scores`` (n, k) float64, ``labels`` the class names, best first.
    From a ``HeadEnsemble`` also, per point: ``entropy`` (the predictive entropy in nats), ``mutual_information`` (the members'
    disagreement, clamped at 0) -- float32 -- and ``votes`` (members whose own best class is the ensemble's, int32); all three
    are ``None`` for a single head."""

    def __init__(self, rowcols: Optional[List[Tuple[int, int]]], indices: np.ndarray, scores: np.ndarray, classes: Sequence[str],
                 stats: Optional[np.ndarray] = None, votes: Optional[np.ndarray] = None):
        self.rowcols = rowcols
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.scores = np.ascontiguousarray(scores, dtype=np.float64)
        if self.indices.ndim != 2 or self.indices.shape != self.scores.shape:
            raise ValueError(f"indices {self.indices.shape} / scores {self.scores.shape} must be equal (n, k) shapes")
        if rowcols is not None and len(rowcols) != self.indices.shape[0]:
            raise ValueError(f"{len(rowcols)} points but {self.indices.shape[0]} prediction rows")
        self.labels: List[List[str]] = [[classes[j] for j in row] for row in self.indices.tolist()]
        self.entropy = self.mutual_information = self.votes = None
        if stats is not None:
            stats = np.asarray(stats, dtype=np.float32).reshape(-1, _lib.MMC_ENSEMBLE_STATS)
            self.votes = np.ascontiguousarray(votes, dtype=np.int32)
            if stats.shape[0] != self.indices.shape[0] or self.votes.shape != (stats.shape[0],):
                raise ValueError(f"stats {stats.shape} / votes {self.votes.shape} do not fit {self.indices.shape[0]} prediction rows")
            self.entropy = stats[:, 0].copy()
            self.mutual_information = np.maximum(stats[:, 2], np.float32(0))

    def __len__(self) -> int:
        return self.indices.shape[0]

    def as_dicts(self) -> Tuple[Dict[Tuple[int, int], List[str]], Dict[Tuple[int, int], List[float]]]:
        """(annotations, scores): the two ``{(row, col): list}`` mappings annotation.py:256-261 fills, in point order; a point
        listed twice keeps its later entry, as the dict assignment there does."""
        if self.rowcols is None:
            raise ValueError("these predictions were made from bare patches: there are no (row, col) keys")
        annotations: Dict[Tuple[int, int], List[str]] = {}
        scores: Dict[Tuple[int, int], List[float]] = {}
        for (row, col), labels, sc in zip(self.rowcols, self.labels, self.scores.tolist()):
            annotations[(row, col)] = labels
            scores[(row, col)] = sc
        return annotations, scores


def _check_k(k) -> int:
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f"k must be an integer >= 1; got {k!r}")
    return int(k)


class _Batcher(PatchBatcher):
    """PatchBatcher whose pass is mmc_classify_patches (mmc_classify_patches_views when the owner has views,
    mmc_ensemble_classify_patches when it holds an ensemble): each flush ends in (points, k) indices and scores in pinned memory,
    for an ensemble also (points, 3) stats and (points,) votes."""

    mean_over_views = True

    def __init__(self, owner: "PointClassifier"):
        super().__init__(owner.backbone, owner.batch_patches)
        self.owner = owner
        self._out: Dict[int, tuple] = {}     # k -> per slot (device idx, device scores, pinned idx, pinned scores)

    def buffers(self, k: int):
        import torch
        if k not in self._out:
            shapes = [((self.cap, k), torch.int32), ((self.cap, k), torch.float32)]
            if self.owner.ensemble is not None:
                shapes += [((self.cap, _lib.MMC_ENSEMBLE_STATS), torch.float32), ((self.cap,), torch.int32)]
            # per slot: the device outputs, then their pinned twins
            self._out[k] = tuple(tuple(torch.empty(sh, dtype=dt, device=self.dev) for sh, dt in shapes) +
                                 tuple(torch.empty(sh, dtype=dt).pin_memory() for sh, dt in shapes) for _ in range(2))
        return self._out[k]

    def _launch(self, slot, patches, fill, k):
        dev = self.buffers(k)[slot]
        dev = dev[: len(dev) // 2]
        self.owner._classify_device(patches, fill, k, dev[0], dev[1], 1 if self.owner.views == (0,) else len(self.owner.views), *dev[2:])

    def _download(self, slot, fill, k):
        bufs = self.buffers(k)[slot]
        half = len(bufs) // 2
        for d, h in zip(bufs[:half], bufs[half:]):
            h[:fill].copy_(d[:fill], non_blocking=True)

    def _fetch(self, slot, count, k):
        bufs = self.buffers(k)[slot]
        return tuple(h[:count].numpy().copy() for h in bufs[len(bufs) // 2:])


class _FeatureBatcher(PatchBatcher):
    """PatchBatcher whose pass appends the backbone's device features to a device ``FeatureSet`` (``cover_images``): nothing comes
    back per pass, the rows stay resident for the one cover call that follows.  One feature buffer per slot, as in
    ``BatchedExtractor``, so the library's graph cache keeps hitting."""

    def __init__(self, owner: "PointClassifier"):
        import torch
        super().__init__(owner.backbone, owner.batch_patches)
        self._fdev = [torch.empty((self.cap, owner.backbone.feature_dim), dtype=torch.float32, device=self.dev) for _ in range(2)]

    def _launch(self, slot, patches, fill, fs):
        feats = self.bb.extract(patches, out=self._fdev[slot][:fill])
        fs.append_device(feats, np.zeros(fill, np.int64))   # (synchronises the stream: the buffer is free when it returns)

    def _download(self, slot, fill, fs):
        pass

    def _fetch(self, slot, count, fs):
        return (np.empty((count, 0), np.float32),)


class PointClassifier:
    """``Backbone`` + ``Predictor`` as one patches -> labels pipeline on the GPU.  ``batch_patches`` bounds the device patch
    buffers of ``classify_image(s)``, as in ``BatchedExtractor``.  ``k`` is the reference's ``predictions_per_point``; more than
    the head has classes gives all of them (the reference's ``[:k]`` slice clamps the same way).

    ``views`` (``backbone.check_views``): ``classify_image(s)`` cut every point once per view code and return one row per point,
    the top-k of the mean of the views' calibrated probabilities (``mmc_classify_patches_views``: fp32, summed in ``views`` order,
    divided by their number).  ``views=(0,)`` is the single fixed window, through the calls and with the bits of before.

    ``predictor`` may be a ``HeadEnsemble``: every pass then goes through ``mmc_ensemble_classify_patches`` (views included) and
    the ``PointPredictions`` carry ``entropy``, ``mutual_information`` and ``votes``.  A single head takes the calls and gives the
    bits it always did."""

    def __init__(self, backbone, predictor, batch_patches: int = 1024, views: Sequence[int] = (0,)):
        if int(batch_patches) < 1:
            raise ValueError(f"batch_patches must be >= 1; got {batch_patches}")
        self.views = check_views(views)
        if int(batch_patches) < len(self.views):
            raise ValueError(f"batch_patches = {batch_patches} cannot hold the {len(self.views)} views of one point")
        if backbone.feature_dim != predictor.input_dim:
            raise ValueError(f"backbone feature_dim {backbone.feature_dim} != predictor input_dim {predictor.input_dim}")
        from .ensemble import HeadEnsemble
        self.backbone = backbone
        self.predictor = predictor
        self.ensemble = predictor if isinstance(predictor, HeadEnsemble) else None
        self.classes = list(predictor.classes)
        self.batch_patches = int(batch_patches)
        self._batcher: Optional[_Batcher] = None     # device buffers are made on first use
        self._feature_batcher: Optional[_FeatureBatcher] = None

    def _k(self, k) -> int:
        return min(_check_k(k), len(self.classes))

    def _classify_device(self, patches, n: int, k: int, idx_dev, scores_dev, g: int = 1, stats_dev=None, votes_dev=None) -> None:
        """mmc_classify_patches on ``n`` device-resident patches into device outputs, asynchronous on the current stream; with
        ``g`` > 1 views per point mmc_classify_patches_views on ``n // g`` points.  An ensemble: mmc_ensemble_classify_patches,
        which also fills ``stats_dev`` (points, 3) and ``votes_dev`` (points,) when given."""
        bb = self.backbone
        if self.ensemble is not None:
            _lib.check(_lib.lib().mmc_ensemble_classify_patches(bb._h, self.ensemble._handle(), patches.data_ptr(), n // g, g, k,
                                                                idx_dev.data_ptr(), scores_dev.data_ptr(),
                                                                None if stats_dev is None else stats_dev.data_ptr(),
                                                                None if votes_dev is None else votes_dev.data_ptr(), 0,
                                                                _current_stream_ptr(bb.device_index)))
            return
        head = self.predictor._head
        if g == 1:
            _lib.check(_lib.lib().mmc_classify_patches(bb._h, head._h, patches.data_ptr(), n, k, idx_dev.data_ptr(),
                                                       scores_dev.data_ptr(), 0, _current_stream_ptr(bb.device_index)))
        else:
            _lib.check(_lib.lib().mmc_classify_patches_views(bb._h, head._h, patches.data_ptr(), n // g, g, k, idx_dev.data_ptr(),
                                                             scores_dev.data_ptr(), 0, _current_stream_ptr(bb.device_index)))

    def topk_device(self, patches, k: int = 1, views_per_point: int = 1, want_uncertainty: bool = False):
        """Device in, device out: contiguous uint8 cuda tensor (N,224,224,3) -> (idx (N/G,k') int32, scores (N/G,k') float32) cuda
        tensors, asynchronous on the current stream (what ``dist.classify_sharded`` gathers).  G = ``views_per_point``: patches
        ``p*G .. p*G+G-1`` are already-cut views of point ``p`` and the row is the top-k of their mean.
        ``want_uncertainty`` (ensembles only): also (stats (N/G,3) float32, votes (N/G,) int32) cuda tensors."""
        import torch
        kk = self._k(k)
        if (not isinstance(patches, torch.Tensor) or not patches.is_cuda or patches.dtype != torch.uint8 or patches.dim() != 4
                or tuple(patches.shape[1:]) != (PATCH, PATCH, 3) or not patches.is_contiguous()):
            raise ValueError("device patches must be a contiguous uint8 cuda tensor (N,224,224,3)")
        if patches.device.index != self.backbone.device_index:
            raise ValueError(f"patches live on {patches.device}, backbone on device {self.backbone.device_index}")
        n = patches.shape[0]
        g = check_views_per_point(n, views_per_point)
        idx = torch.empty((n // g, kk), dtype=torch.int32, device=patches.device)
        scores = torch.empty((n // g, kk), dtype=torch.float32, device=patches.device)
        if want_uncertainty:
            if self.ensemble is None:
                raise ValueError("want_uncertainty needs a HeadEnsemble: a single head has no members to disagree")
            stats = torch.empty((n // g, _lib.MMC_ENSEMBLE_STATS), dtype=torch.float32, device=patches.device)
            votes = torch.empty((n // g,), dtype=torch.int32, device=patches.device)
            if n:
                self._classify_device(patches, n, kk, idx, scores, g, stats, votes)
            return idx, scores, stats, votes
        if n:
            self._classify_device(patches, n, kk, idx, scores, g)
        return idx, scores

    def classify_patches(self, patches, k: int = 1, views_per_point: int = 1) -> PointPredictions:
        """patches: (N,224,224,3) uint8 -- numpy (host) or a cuda tensor on the backbone's device.  ``views_per_point`` = G:
        patches ``p*G .. p*G+G-1`` are already-cut views of point ``p``; one prediction row per point, from their mean."""
        kk = self._k(k)
        if isinstance(patches, np.ndarray):
            p = np.ascontiguousarray(patches)
            if p.dtype != np.uint8 or p.ndim != 4 or p.shape[1:] != (PATCH, PATCH, 3):
                raise ValueError(f"patches must be uint8 (N,{PATCH},{PATCH},3); got {p.dtype} {p.shape}")
            n = p.shape[0]
            g = check_views_per_point(n, views_per_point)
            idx = np.empty((n // g, kk), dtype=np.int32)
            scores = np.empty((n // g, kk), dtype=np.float32)
            if self.ensemble is not None:
                stats = np.empty((n // g, _lib.MMC_ENSEMBLE_STATS), dtype=np.float32)
                votes = np.empty(n // g, dtype=np.int32)
                if n:
                    bb = self.backbone
                    _lib.check(_lib.lib().mmc_ensemble_classify_patches(bb._h, self.ensemble._handle(), p.ctypes.data, n // g, g, kk,
                                                                        idx.ctypes.data, scores.ctypes.data, stats.ctypes.data,
                                                                        votes.ctypes.data, _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST,
                                                                        _current_stream_ptr(bb.device_index)))
                return PointPredictions(None, idx, scores, self.classes, stats, votes)
            if n:
                bb, head = self.backbone, self.predictor._head
                flags = _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST
                if g == 1:
                    _lib.check(_lib.lib().mmc_classify_patches(bb._h, head._h, p.ctypes.data, n, kk, idx.ctypes.data, scores.ctypes.data,
                                                               flags, _current_stream_ptr(bb.device_index)))
                else:
                    _lib.check(_lib.lib().mmc_classify_patches_views(bb._h, head._h, p.ctypes.data, n // g, g, kk, idx.ctypes.data,
                                                                     scores.ctypes.data, flags, _current_stream_ptr(bb.device_index)))
            return PointPredictions(None, idx, scores, self.classes)
        try:
            import torch
            is_tensor = isinstance(patches, torch.Tensor)
        except ImportError:
            is_tensor = False
        if not is_tensor:
            raise TypeError("patches must be a numpy array or a torch tensor")
        out = self.topk_device(patches, kk, views_per_point, want_uncertainty=self.ensemble is not None)
        return PointPredictions(None, *(t.cpu().numpy() for t in out[:2]), self.classes, *(t.cpu().numpy() for t in out[2:]))

    def classify_images(self, images: Iterable[np.ndarray], rowcols_per_image: Iterable[Sequence[Tuple[int, int]]],
                        k: int = 1) -> List[PointPredictions]:
        """One ``PointPredictions`` per image, rows in ``rowcols`` order (empty for an image without points).  Inputs are checked
        as ``BatchedExtractor`` checks them, all of them before the GPU is touched; points of consecutive images share passes."""
        kk = self._k(k)
        prepared = [prepare_image(i, im, rc) for i, (im, rc) in enumerate(zip(images, rowcols_per_image))]
        if self._batcher is None:
            self._batcher = _Batcher(self)
        out, points = self._batcher._run([im for im, _ in prepared], [rc for _, rc in prepared], ctx=kk, views=self.views)
        res = []
        for o, rc in zip(out, points):
            pts = [(int(r), int(c)) for r, c in rc]
            if o is None:
                empty = () if self.ensemble is None else (np.zeros((0, _lib.MMC_ENSEMBLE_STATS), np.float32), np.zeros(0, np.int32))
                res.append(PointPredictions(pts, np.zeros((0, kk), np.int32), np.zeros((0, kk), np.float64), self.classes, *empty))
            else:
                res.append(PointPredictions(pts, o[0], o[1], self.classes, *o[2:]))
        return res

    def classify_image(self, image: np.ndarray, rowcols: Sequence[Tuple[int, int]], k: int = 1) -> PointPredictions:
        """annotation.py:239-261 for one image: ``classify_image(loaded_image, rowcols, k).as_dicts()`` are its ``annotations`` /
        ``scores`` entries."""
        return self.classify_images([image], [list(rowcols)], k)[0]

    def cover_images(self, images: Iterable[np.ndarray], rowcols_per_image: Iterable[Sequence[Tuple[int, int]]], group_of_image=None,
                     train_prior=None, strength: float = 1.0, iters: int = 20, k: int = 0):
        """Images + points -> ``cover.CoverEstimate``: percent cover per image, or per run of consecutive images that share an id in
        ``group_of_image`` (a transect, a source), with ``.topk`` (``k`` > 0) the labels of every point under its group's adapted
        prior, rows in image and ``rowcols`` order.  The backbone's features go from each pass into a device ``FeatureSet`` and
        one ``mmc_head_cover_set`` runs over it: neither features nor probabilities visit the host.  With ``views`` a point's views
        are its G rows.  ``train_prior`` / ``strength`` / ``iters`` / ``k``: ``cover.estimate_cover``.  Host arguments are checked
        before the GPU is touched; ``.groups`` holds the group ids (image indices without ``group_of_image``)."""
        from .cover import check_cover_arguments, estimate_cover, image_groups
        from .featureset import FeatureSet
        if self.ensemble is not None:
            raise ValueError("cover_images takes a single head; for an ensemble pass its float32 probabilities to estimate_cover: "
                             "estimate_cover(ens.topk(features, 1, want_proba=True)[2], None, group_offsets, ...)")
        prepared = [prepare_image(i, im, rc) for i, (im, rc) in enumerate(zip(images, rowcols_per_image))]
        offsets, ids = image_groups([len(rc) for _, rc in prepared], group_of_image)
        n, g = int(offsets[-1]), len(self.views)
        check_cover_arguments(n, len(self.classes), offsets, train_prior, strength, iters, k)
        fs = FeatureSet(self.backbone.feature_dim, [0], device=self.backbone.device_index, reserve=n * g)
        try:
            if n:
                if self._feature_batcher is None:
                    self._feature_batcher = _FeatureBatcher(self)
                self._feature_batcher._run([im for im, _ in prepared], [rc for _, rc in prepared], ctx=fs, views=self.views)
                est = estimate_cover(self.predictor, fs, offsets, train_prior, strength, iters, k, views_per_point=g)
            else:
                est = estimate_cover(self.predictor, np.zeros((0, self.predictor.input_dim), np.float32), offsets, train_prior, strength,
                                     iters, k)
        finally:
            fs.close()
        if est.topk is not None:
            est.topk = PointPredictions([(int(r), int(c)) for _, rc in prepared for r, c in rc], est.topk.indices, est.topk.scores,
                                        self.classes)
        est.groups = ids
        return est
