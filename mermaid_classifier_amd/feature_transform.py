"""``FeatureTransform``: a fitted linear transform of the backbone features -- per-feature standardisation, PCA reduction or PCA
whitening, on total or pooled within-class scatter -- fitted on a resident ``FeatureSet``, applied on the device into another
resident set, and folded into the head's first Linear layer at calibration time.

The reference trains its MLP on the raw pooled activations (``mermaid_classifier/pyspacer/trainer.py:118-145``);
``docs/research/hidden-layer-experiments.md`` section 5 names the feature representation as the next thing to vary.  No reference
counterpart: the device stage is defined in ``include/mmc.h`` ("feature transforms", ``csrc/features.hip``), the host algebra here:

``fit``     ``mmc_featureset_moments`` (counts, fp64 means and sums of squared deviations, per class and global); for ``pca`` /
            ``whiten`` also ``mmc_featureset_scatter`` about the fp32 cast of those means, divided by n, then
            ``numpy.linalg.eigh`` in float64 on the host (dim x dim: not the hot path).  Eigenvalues descending; each
            eigenvector's sign makes its largest-magnitude component positive (ties: the lowest index).
``apply``   ``mmc_featureset_transform``: ``(x - mean) . components^T`` in fp32 into a new resident set; the rows never visit the host.
``fold``    ``W1' = W1 . components``, ``b1' = b1 - W1' . mean`` in float64, rounded to fp32 once: the head then takes RAW features, so
            ``model.pt`` / ``model.json``, ``Predictor``, ``PointClassifier`` and every validation entry are unchanged.

``train_classifier`` / ``train_sweep`` / ``train_and_validate`` take ``transform=`` (a fitted ``FeatureTransform`` or a dict of
``fit`` keyword arguments) and return folded models.  Whether any of these transforms improves accuracy or cover R^2 on reef data
has NOT been measured.  No CPU fallback for ``fit`` from a set and ``apply``; a fitted transform (``fold``, ``transform_rows``,
pickling) needs no device.
"""

from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr
from .featureset import FeatureSet

__all__ = ["FeatureTransform", "KINDS", "SCATTERS"]

KINDS = ("standardize", "pca", "whiten")
SCATTERS = ("total", "within")


def _check_fit_args(dim: int, kind, n_components, eps, scatter) -> Tuple[int, float]:
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    if scatter not in SCATTERS:
        raise ValueError(f"scatter must be one of {SCATTERS}, got {scatter!r}")
    try:
        eps_f = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"eps must be a positive finite number, got {eps!r}")
    if not (np.isfinite(eps_f) and eps_f > 0):
        raise ValueError(f"eps must be a positive finite number, got {eps!r}")
    if n_components is None:
        m = int(dim)
    else:
        if isinstance(n_components, bool) or int(n_components) != n_components or not 1 <= int(n_components) <= dim:
            raise ValueError(f"n_components must be an integer in [1, {dim}], got {n_components!r}")
        m = int(n_components)
        if kind == "standardize" and m != dim:
            raise ValueError("n_components applies to kind 'pca' / 'whiten': 'standardize' keeps every feature")
    return m, eps_f


def eigen_basis(cov: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """-> (eigenvalues descending, V^T with one eigenvector per ROW) of the symmetric float64 matrix ``cov``; each eigenvector's
    sign makes its largest-magnitude component positive, the lowest index among equal magnitudes."""
    lam, V = np.linalg.eigh(np.asarray(cov, np.float64))
    order = np.argsort(-lam, kind="stable")
    lam, Vt = lam[order], V[:, order].T.copy()
    lead = np.argmax(np.abs(Vt), axis=1)                          # the first maximum
    sign = np.where(Vt[np.arange(len(Vt)), lead] < 0, -1.0, 1.0)
    return lam, Vt * sign[:, None]


class FeatureTransform:
    """``y = (x - mean_) . components_^T``.  Attributes: ``kind``, ``scatter``, ``eps``, ``dim`` (input width), ``n_components``
    (output width m), ``mean_`` (dim,) float64 -- always the GLOBAL mean --, ``components_`` (m, dim) float64,
    ``explained_variance_`` (m,) float64 (the variances / eigenvalues the scaling was made from), ``counts_`` (K,) int64,
    ``class_means_`` (K, dim) float64, ``n_rows_``.  Make one with ``fit`` (device) or ``from_statistics`` (host)."""

    def __init__(self, kind: str, mean, components, explained_variance, *, scatter: str = "total", eps: float = 1e-3,
                 counts=None, class_means=None):
        self.kind, self.scatter, self.eps = kind, scatter, float(eps)
        self.mean_ = np.array(mean, dtype=np.float64)
        self.components_ = np.array(components, dtype=np.float64)
        self.explained_variance_ = np.array(explained_variance, dtype=np.float64)
        if self.mean_.ndim != 1 or self.components_.ndim != 2 or self.components_.shape[1] != self.mean_.shape[0]:
            raise ValueError(f"mean {self.mean_.shape} and components {self.components_.shape} do not fit")
        self.counts_ = None if counts is None else np.array(counts, dtype=np.int64)
        self.class_means_ = None if class_means is None else np.array(class_means, dtype=np.float64)
        self.n_rows_ = None if counts is None else int(self.counts_.sum())

    @property
    def dim(self) -> int:
        return int(self.components_.shape[1])

    @property
    def n_components(self) -> int:
        return int(self.components_.shape[0])

    # ---- fitting ----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_statistics(cls, kind: str, counts, mean, m2, scatter_matrix=None, *, n_components: Optional[int] = None,
                        eps: float = 1e-3, scatter: str = "total") -> "FeatureTransform":
        """The host half of ``fit``: ``counts`` (K,), ``mean`` / ``m2`` ((K + 1), dim) as ``mmc_featureset_moments`` defines them
        (slot K global) and, for ``pca`` / ``whiten``, the dim x dim ``scatter_matrix`` of ``mmc_featureset_scatter`` (about the
        global mean for ``scatter="total"``, about the class means for ``"within"``)."""
        counts = np.asarray(counts, np.int64)
        mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
        K, dim = len(counts), mean.shape[1]
        if mean.shape != (K + 1, dim) or m2.shape != mean.shape:
            raise ValueError(f"mean / m2 must be ({K + 1}, dim); got {mean.shape} and {m2.shape}")
        m, eps = _check_fit_args(dim, kind, n_components, eps, scatter)
        n = int(counts.sum())
        if n < 2:
            raise ValueError(f"a transform needs at least 2 rows, got {n}")
        if kind == "standardize":
            var = (m2[K] if scatter == "total" else m2[:K].sum(axis=0)) / n
            comps = np.diag(1.0 / np.sqrt(var + eps * var.mean()))
            ev = var
        else:
            S = np.asarray(scatter_matrix, np.float64)
            if S.shape != (dim, dim):
                raise ValueError(f"scatter_matrix must be ({dim}, {dim}), got {S.shape}")
            lam, Vt = eigen_basis(S / n)
            comps, ev = Vt[:m], lam[:m]
            if kind == "whiten":
                lam0 = np.maximum(lam, 0.0)   # a rank-deficient scatter's smallest eigenvalues round below zero
                comps = comps / np.sqrt(lam0[:m] + eps * lam0.mean())[:, None]
        return cls(kind, mean[K], comps, ev, scatter=scatter, eps=eps, counts=counts, class_means=mean[:K])

    @classmethod
    def fit(cls, fs: FeatureSet, kind: str, *, n_components: Optional[int] = None, eps: float = 1e-3, scatter: str = "total",
            rows: Optional[Tuple[int, int]] = None) -> "FeatureTransform":
        """Fit on rows ``rows = (first, n)`` of the resident set ``fs`` (None: all of it).  ``kind``: ``"standardize"``
        (``components_ = diag(1 / sqrt(var_j + eps mean(var)))``), ``"pca"`` (``V^T``) or ``"whiten"``
        (``diag(1 / sqrt(lambda + eps mean(lambda))) V^T``), the last two cut to ``n_components``.  ``scatter="within"`` takes the
        variances / the scatter matrix about the class means (pooled within-class); the transform still centres on the global mean.
        Every argument error (unknown ``kind`` / ``scatter``, ``eps <= 0``, ``n_components`` outside [1, dim], fewer than 2 rows)
        is raised before a device is touched."""
        if not isinstance(fs, FeatureSet):
            raise ValueError(f"fs must be a FeatureSet, got {type(fs).__name__}")
        _check_fit_args(fs.dim, kind, n_components, eps, scatter)
        total = len(fs)
        first, n = (0, total) if rows is None else (int(rows[0]), int(rows[1]))
        if first < 0 or n < 0 or first + n > total:
            raise ValueError(f"rows [{first}, {first + n}) outside the set's {total} rows")
        if n < 2:
            raise ValueError(f"a transform needs at least 2 rows, got {n}")
        if kind != "standardize" and fs.dim > _lib.MMC_SCATTER_MAX_DIM:
            raise ValueError(f"the set has {fs.dim} features; the scatter stage takes at most {_lib.MMC_SCATTER_MAX_DIM}")
        counts, mean, m2 = moments(fs, first, n)
        S = None
        if kind != "standardize":
            K = len(counts)
            centres = mean[K] if scatter == "total" else mean[:K]
            S = scatter_matrix(fs, centres.astype(np.float32), first, n)
        return cls.from_statistics(kind, counts, mean, m2, S, n_components=n_components, eps=eps, scatter=scatter)

    # ---- using ------------------------------------------------------------------------------------------------------------
    def device_operands(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (centre (dim,), T (m, dim)) float32: what ``apply`` hands to ``mmc_featureset_transform``."""
        return (np.ascontiguousarray(self.mean_.astype(np.float32)), np.ascontiguousarray(self.components_.astype(np.float32)))

    def apply(self, fs: FeatureSet) -> FeatureSet:
        """-> a new resident ``FeatureSet`` of width ``n_components`` with ``fs``'s classes and labels: every row of ``fs``
        through ``mmc_featureset_transform``, on ``fs``'s device.  The caller closes it."""
        if not isinstance(fs, FeatureSet):
            raise ValueError(f"fs must be a FeatureSet, got {type(fs).__name__}")
        if fs.dim != self.dim:
            raise ValueError(f"the feature set has {fs.dim} features, the transform takes {self.dim}")
        n = len(fs)
        out = FeatureSet(self.n_components, fs.classes, device=fs.device, reserve=n)
        if n:
            centre, T = self.device_operands()
            _lib.check(_lib.lib().mmc_featureset_transform(fs._handle(), 0, n, centre.ctypes.data, T.ctypes.data, self.n_components,
                                                           out._handle(), _lib.MMC_IN_HOST, _current_stream_ptr(fs.device_index)))
        return out

    def transform_rows(self, X) -> np.ndarray:
        """Host rows (n, dim) -> (n, m) in float64: the definition ``apply`` is held to, for small inputs and checks."""
        X = np.asarray(X, np.float64)
        if X.ndim != 2 or X.shape[1] != self.dim:
            raise ValueError(f"X must be (N, {self.dim}); got {X.shape}")
        return (X - self.mean_) @ self.components_.T

    def fold(self, weights: Sequence[np.ndarray], biases: Sequence[np.ndarray]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """Parameters of a head trained on transformed features -> parameters of the same function of RAW features: in float64
        ``W1' = W1 . components_`` and ``b1' = b1 - W1' . mean_``, each rounded to float32 once; the other layers are copied."""
        W1 = np.asarray(weights[0], np.float64)
        if W1.ndim != 2 or W1.shape[1] != self.n_components:
            raise ValueError(f"the first layer takes {W1.shape[-1]} features, the transform writes {self.n_components}")
        Wf = W1 @ self.components_
        bf = np.asarray(biases[0], np.float64) - Wf @ self.mean_
        return ([Wf.astype(np.float32)] + [np.array(w, dtype=np.float32) for w in weights[1:]],
                [bf.astype(np.float32)] + [np.array(v, dtype=np.float32) for v in biases[1:]])


def moments(fs: FeatureSet, first: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``mmc_featureset_moments`` on rows [first, first + n) of ``fs`` -> (counts (K,) int64, mean (K + 1, dim), m2 (K + 1, dim))."""
    n = len(fs) - int(first) if n is None else int(n)
    K = len(fs.classes)
    counts = np.zeros(K, np.int64)
    mean = np.zeros((K + 1, fs.dim), np.float64)
    m2 = np.zeros((K + 1, fs.dim), np.float64)
    _lib.check(_lib.lib().mmc_featureset_moments(fs._handle(), int(first), n, counts.ctypes.data, mean.ctypes.data, m2.ctypes.data,
                                                 _lib.MMC_OUT_HOST, _current_stream_ptr(fs.device_index)))
    return counts, mean, m2


def scatter_matrix(fs: FeatureSet, centres, first: int = 0, n: Optional[int] = None) -> np.ndarray:
    """``mmc_featureset_scatter`` on rows [first, first + n) of ``fs`` -> (dim, dim) float64.  ``centres``: float32 (dim,) for the
    scatter about one centre, (K, dim) for the pooled scatter about each row's class centre."""
    n = len(fs) - int(first) if n is None else int(n)
    c = np.ascontiguousarray(np.asarray(centres, dtype=np.float32))
    if c.shape == (fs.dim,):
        by_label = 0
    elif c.shape == (len(fs.classes), fs.dim):
        by_label = 1
    else:
        raise ValueError(f"centres must be ({fs.dim},) or ({len(fs.classes)}, {fs.dim}); got {c.shape}")
    S = np.zeros((fs.dim, fs.dim), np.float64)
    _lib.check(_lib.lib().mmc_featureset_scatter(fs._handle(), int(first), n, c.ctypes.data, by_label, S.ctypes.data,
                                                 _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST, _current_stream_ptr(fs.device_index)))
    return S


def resolve(transform, train: FeatureSet) -> FeatureTransform:
    """``train_classifier``'s ``transform`` argument -> a fitted transform: itself, or ``FeatureTransform.fit(train, **transform)``."""
    if isinstance(transform, FeatureTransform):
        ft = transform
    elif isinstance(transform, dict):
        ft = FeatureTransform.fit(train, **transform)
    else:
        raise ValueError(f"transform must be a FeatureTransform or a dict of fit arguments, got {type(transform).__name__}")
    if ft.dim != train.dim:
        raise ValueError(f"the transform takes {ft.dim} features, the splits have {train.dim}")
    return ft
