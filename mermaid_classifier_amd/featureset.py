"""``FeatureSet``: one labelled split (train, ref or val) resident on the MI355X.

The reference streams every split from disk once per epoch (``labels.train.load_data_in_batches``, ``mermaid_classifier/
pyspacer/trainer.py:141-145``; the ref / val streams of ``_calc_acc_batched`` :295-307, ``_calc_acc_and_log_loss_batched``
:309-342 and ``_calibrate_in_batches`` :344-396) because a CPU box cannot hold N x dim floats.  A set is filled once -- from host
arrays (``append``) or from rows that are already on the device, such as ``Backbone.extract``'s output (``append_device``) -- and
``TorchMLPClassifier.partial_fit_rows``, ``calibration.evaluate`` and ``calibration.calibrate`` then read it in place
(``mmc_featureset_*``, csrc/featureset.hip).  fp32 rows; labels are stored as indices into ``classes``.

The device handle is created by the first call that needs it, so argument errors (wrong width, unknown labels) surface without
a device.  No CPU fallback.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr, _device_index

__all__ = ["FeatureSet"]


class FeatureSet:
    """``FeatureSet(dim, classes, device=0, reserve=0)``: rows of ``dim`` float32 features with labels out of ``classes``
    (stored sorted and unique, as ``TorchMLPClassifier.classes_`` is).  ``reserve`` rows are allocated up front; beyond that
    the capacity grows geometrically with a device-to-device copy."""

    def __init__(self, dim: int, classes, device=0, reserve: int = 0):
        self.dim = int(dim)
        self.classes = np.unique(np.asarray(classes))
        if self.dim < 1:
            raise ValueError(f"dim must be positive, got {dim!r}")
        if self.classes.size < 1:
            raise ValueError("classes is empty")
        if int(reserve) < 0:
            raise ValueError(f"reserve must be >= 0, got {reserve!r}")
        self.device = device
        self.device_index = _device_index(device)
        self._reserve = int(reserve)
        self._h = None

    # ---- handle ---------------------------------------------------------------------------------------------------
    def _handle(self) -> C.c_void_p:
        if self._h is None:
            h = C.c_void_p()
            _lib.check(_lib.lib().mmc_featureset_create(self.dim, len(self.classes), self.device_index, self._reserve, C.byref(h)))
            self._h = h
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().mmc_featureset_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return 0 if self._h is None else int(_lib.lib().mmc_featureset_rows(self._h))

    # ---- filling --------------------------------------------------------------------------------------------------
    def _label_indices(self, y, n: int) -> np.ndarray:
        y = np.asarray(y)
        if y.shape != (n,):
            raise ValueError(f"y has shape {y.shape}, expected ({n},)")
        idx = np.searchsorted(self.classes, y)
        if n and not np.array_equal(self.classes[np.minimum(idx, len(self.classes) - 1)], y):
            bad = set(y.tolist()) - set(self.classes.tolist())
            raise ValueError(f"Labels {sorted(bad)} are not in classes {self.classes.tolist()}.")
        return np.ascontiguousarray(idx.astype(np.int32))

    def append(self, X, y) -> "FeatureSet":
        """Host rows ``X`` (n, dim) with labels ``y`` (n,) out of ``classes``.
        Patch views as augmentation need nothing more: ``append(F, np.repeat(y, G))`` of one image's
        ``BatchedExtractor.extract_images(..., views=views)`` rows ``F`` (G = len(views), point-major) adds G rows per annotation.
        Keep the views of one annotation in one split: split by annotation first, expand to views afterwards."""
        X_arr = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        if X_arr.ndim != 2:
            raise ValueError(f"X must be 2D, got shape {X_arr.shape}")
        if X_arr.shape[1] != self.dim:
            raise ValueError(f"X has {X_arr.shape[1]} features, expected {self.dim}")
        yi = self._label_indices(y, X_arr.shape[0])
        _lib.check(_lib.lib().mmc_featureset_append(self._handle(), X_arr.ctypes.data, yi.ctypes.data, X_arr.shape[0],
                                                    _lib.MMC_IN_HOST, _current_stream_ptr(self.device_index)))
        return self

    def append_device(self, features, y) -> "FeatureSet":
        """Rows that are already on the set's device: a contiguous float32 cuda tensor (n, dim), e.g. what ``Backbone.extract``
        returns for device patches.  The rows never visit the host; the labels ``y`` are host values."""
        import torch
        if not isinstance(features, torch.Tensor) or not features.is_cuda:
            raise ValueError("features must be a cuda tensor (host rows go through append)")
        if features.device.index != self.device_index:
            raise ValueError(f"features live on {features.device}, the set on device {self.device_index}")
        if features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] != self.dim or not features.is_contiguous():
            raise ValueError(f"features must be a contiguous float32 tensor (n, {self.dim}); got {features.dtype} {tuple(features.shape)}"
                             f"{'' if features.is_contiguous() else ' (not contiguous)'}")
        n = int(features.shape[0])
        yi = self._label_indices(y, n)
        _lib.check(_lib.lib().mmc_featureset_append(self._handle(), features.data_ptr(), yi.ctypes.data, n, 0,
                                                    _current_stream_ptr(self.device_index)))
        return self

    # ---- reading back ---------------------------------------------------------------------------------------------
    def read(self, first: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """-> (X, y) of rows [first, first + n) on the host (``n=None``: to the end); ``y`` as labels out of ``classes``."""
        total = len(self)
        first = int(first)
        n = total - first if n is None else int(n)
        if first < 0 or n < 0 or first + n > total:
            raise ValueError(f"rows [{first}, {first + n}) outside the set's {total} rows")
        X = np.empty((n, self.dim), np.float32)
        yi = np.empty((n,), np.int32)
        if n:
            _lib.check(_lib.lib().mmc_featureset_read(self._h, first, n, X.ctypes.data, yi.ctypes.data,
                                                      _current_stream_ptr(self.device_index)))
        return X, self.classes[yi]

    def _check_against(self, clf) -> None:
        """The set must carry the classifier's classes and width: its label indices are the classifier's."""
        if not np.array_equal(self.classes, clf.classes_):
            raise ValueError(f"the feature set's classes {self.classes.tolist()} differ from classes_ {np.asarray(clf.classes_).tolist()}")
        if self.dim != clf.n_features_in_:
            raise ValueError(f"the feature set has {self.dim} features, expected {clf.n_features_in_}")
