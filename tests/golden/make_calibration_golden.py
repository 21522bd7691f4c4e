"""Generate tests/golden/calibration_fixture.npz: sklearn's Platt calibration (``_SigmoidCalibration``, the per-class fit
``_fit_calibrator(..., "sigmoid")`` runs) and ``log_loss`` / ``accuracy_score`` on seeded float64 inputs.

    python tests/golden/make_calibration_golden.py      (needs scikit-learn; written with 1.7.2)

Sets (each a multiclass problem: scores S [N][K] float64, labels y in [0, K)):
  main   4000 x 12 softmax probabilities of seeded logits, labels drawn from a sharpened version of them
  deg    4000 x 6: col 0 constant zero, col 1 probabilities * 1e-30, col 2 a single positive, col 3 no positives,
         col 4 decision values with |F| >= 30, col 5 ordinary probabilities
  allpos 200 x 3, every label 0: class 0 all positives, classes 1 and 2 none
For each set: a / b of sklearn (float64); the calibrated probabilities follow from them (calibrated_proba below is
_CalibratedClassifier.predict_proba: sigmoid per class, row-normalised, the overshoot clip).  Plus ll_P [500][12] / ll_y with sklearn's log_loss(labels=range(12)) and
accuracy_score of its argmax.
"""

from pathlib import Path

import numpy as np
import sklearn
from scipy.special import expit
from sklearn.calibration import _SigmoidCalibration
from sklearn.metrics import accuracy_score, log_loss


def softmax(z):
    z = z - z.max(1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(1, keepdims=True)


def calibrated_proba(S, a, b):
    c = expit(-(a[None, :] * S + b[None, :]))
    d = c.sum(1, keepdims=True)
    p = np.divide(c, d, out=np.full_like(c, 1.0 / c.shape[1]), where=d != 0)
    p[(1.0 < p) & (p <= 1.0 + 1e-5)] = 1.0
    return p


def fit(S, y):
    a, b = np.empty(S.shape[1]), np.empty(S.shape[1])
    for k in range(S.shape[1]):
        cal = _SigmoidCalibration().fit(S[:, k], (y == k).astype(np.int64))
        a[k], b[k] = cal.a_, cal.b_
    return a, b


def main():
    rng = np.random.default_rng(20261016)
    out = {"sklearn_version": np.array(sklearn.__version__)}

    z = rng.normal(0.0, 2.0, size=(4000, 12))
    S = softmax(z)
    y = np.array([rng.choice(12, p=q) for q in softmax(1.5 * z)], dtype=np.int32)
    sets = {"main": (S, y)}

    n = 4000
    p = softmax(rng.normal(0.0, 1.5, size=(n, 6)))
    D = np.empty((n, 6))
    D[:, 0] = 0.0
    D[:, 1] = p[:, 1] * 1e-30
    D[:, 2] = p[:, 2]
    D[:, 3] = p[:, 3]
    D[:, 4] = rng.normal(0.0, 15.0, size=n)
    D[:, 4][np.argmax(np.abs(D[:, 4]))] = 45.0   # |F| >= 30 guaranteed
    D[:, 5] = p[:, 5]
    yd = rng.choice([0, 1, 4, 5], size=n, p=[0.2, 0.3, 0.25, 0.25]).astype(np.int32)
    yd[rng.choice(n)] = 2                        # a single positive for class 2, none for class 3
    pos4 = D[:, 4] > 5.0
    yd[pos4 & (yd != 2)] = 4                     # a decision value that carries signal
    sets["deg"] = (D, yd)

    sets["allpos"] = (softmax(rng.normal(0.0, 1.0, size=(200, 3))), np.zeros(200, np.int32))

    for name, (S_, y_) in sets.items():
        a, b = fit(S_, y_)
        out[f"{name}_S"], out[f"{name}_y"] = S_, y_
        out[f"{name}_a"], out[f"{name}_b"] = a, b

    P = softmax(rng.normal(0.0, 3.0, size=(500, 12)))
    P[0, 3] = 0.0                                # a zero probability on the true class exercises the clip
    P[0] /= P[0].sum()
    yl = rng.integers(0, 12, size=500).astype(np.int32)
    yl[0] = 3
    out["ll_P"], out["ll_y"] = P, yl
    out["ll_log_loss"] = np.array(log_loss(yl, P, labels=list(range(12))))
    out["ll_accuracy"] = np.array(accuracy_score(yl, P.argmax(1)))

    path = Path(__file__).resolve().parent / "calibration_fixture.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
