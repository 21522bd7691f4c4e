"""Wall time of the three feature-transform entries at n x dim resident rows, beside the same steps in float64 numpy on the host.

    python tools/feature_transform_cost.py [--rows 200000] [--dim 1280] [--out profiles/feature_transform_cost.txt]

Each step runs once, in a child process of its own under `timeout` (the parent stops at the first child that fails): the child fills a
resident set with seeded non-negative correlated rows, warms the step's kernels on 512 rows, then times ONE call with the host clock
(every entry ends in a stream synchronisation).  The host figures are context, not a target: the parent commit has no device path.
"""

from __future__ import annotations

import argparse
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

K = 40
FP32_MATRIX_ROOF = 157e12   # FLOP/s, exact-f32 MFMA peak of an MI355X
STEPS = {"moments": 240, "scatter": 240, "transform": 240, "host": 540}   # seconds allowed per child


def rows_block(n: int, dim: int, seed: int):
    rng = np.random.default_rng(seed)
    mix = rng.normal(0, 1, (64, dim)).astype(np.float32)
    base = rng.uniform(3.0, 9.0, dim).astype(np.float32)
    X = base + rng.normal(0, 1, (n, 64)).astype(np.float32) @ mix / 8 + 0.3 * rng.normal(0, 1, (n, dim)).astype(np.float32)
    return np.maximum(X, 0, out=X), rng.integers(0, K, n)


def filled_set(n: int, dim: int):
    from mermaid_classifier_amd import FeatureSet
    fs = FeatureSet(dim, np.arange(K), reserve=n)
    for first in range(0, n, 20000):                       # the same 20 000 rows over and over would make the scatter rank-poor
        X, y = rows_block(min(20000, n - first), dim, seed=first)
        fs.append(X, y)
    return fs


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def step(name: str, n: int, dim: int) -> None:
    from mermaid_classifier_amd import FeatureSet
    from mermaid_classifier_amd import feature_transform as ftm
    if name == "host":
        import os
        threads = min(16, os.cpu_count() or 1)
        X = np.concatenate([rows_block(min(20000, n - f), dim, seed=f)[0] for f in range(0, n, 20000)])
        X64, t_cast = timed(lambda: X.astype(np.float64))

        def host_moments():
            mu = X64.mean(axis=0)
            return mu, ((X64 - mu) ** 2).sum(axis=0)

        (mean, m2), t_mom = timed(host_moments)
        Xc, t_c = timed(lambda: X64 - mean)
        S, t_sc = timed(lambda: Xc.T @ Xc)
        T = np.linalg.eigh(S / n)[1].T.copy()
        Y, t_tr = timed(lambda: Xc @ T.T)
        print(f"host float64 numpy ({threads} threads; context, not a target): cast to float64 {t_cast * 1e3:.1f} ms; "
              f"global moments {t_mom * 1e3:.1f} ms; centre {t_c * 1e3:.1f} ms + scatter {t_sc * 1e3:.1f} ms; "
              f"transform (m = dim) {t_tr * 1e3:.1f} ms", flush=True)
        return
    fs = filled_set(n, dim)
    small = FeatureSet(dim, np.arange(K)).append(*rows_block(512, dim, seed=1))
    counts, mean, m2 = ftm.moments(small)
    if name == "moments":
        _, t = timed(lambda: ftm.moments(fs))
        print(f"mmc_featureset_moments   {n} x {dim}, K = {K}: {t * 1e3:.2f} ms   ({n * dim * 4 / t / 1e9:.0f} GB/s of rows x dim x 4 bytes;"
              f" the rows are read four times)", flush=True)
    elif name == "scatter":
        ftm.scatter_matrix(small, mean[K].astype(np.float32))
        c = ftm.moments(fs)[1]
        for label, centres in (("one centre", c[K]), ("by label", c[:K])):
            _, t = timed(lambda: ftm.scatter_matrix(fs, centres.astype(np.float32)))
            tiles = -(-dim // 128)
            pairs = tiles * (tiles + 1) // 2
            issued = 2.0 * (-(-n // 16) * 16) * pairs * 128 * 128          # what the MFMAs of the launched tile pairs execute
            print(f"mmc_featureset_scatter   {n} x {dim}, {label}: {t * 1e3:.2f} ms wall (upload of the centres, both launches, "
                  f"{dim * dim * 8 / 1e6:.0f} MB copied back); {issued / t / 1e12:.1f} TFLOP/s issued = "
                  f"{issued / t / FP32_MATRIX_ROOF:.3f} of the 157 TF fp32-matrix roof; as a full {dim} x {dim} product "
                  f"(2 n dim^2) {2.0 * n * dim * dim / t / 1e12:.1f} TFLOP/s", flush=True)
    elif name == "transform":
        ft = ftm.FeatureTransform("pca", mean[K], np.eye(dim), np.ones(dim))
        ft.apply(small).close()
        for m in (dim, 256):
            ftm_m = ftm.FeatureTransform("pca", mean[K], np.eye(dim)[:m], np.ones(m))
            out, t = timed(lambda: ftm_m.apply(fs))
            out.close()
            print(f"FeatureTransform.apply   {n} x {dim} -> m = {m}: {t * 1e3:.2f} ms wall (allocation of the new set included); "
                  f"{2.0 * n * dim * m / t / 1e12:.1f} TFLOP/s", flush=True)
    fs.close()
    small.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=1280)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.rows, args.dim)
        return 0
    lines = [f"# python tools/feature_transform_cost.py --rows {args.rows} --dim {args.dim}",
             "# one timed call per step, each step in its own process; host clock around calls that end in a stream synchronisation"]
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--step", name,
               "--rows", str(args.rows), "--dim", str(args.dim)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(run.stdout, end="", flush=True)
        lines += [ln for ln in run.stdout.splitlines() if "amdgpu.ids" not in ln]   # (a libdrm notice, not a result)
        if run.returncode != 0:
            print(f"step {name} ended with status {run.returncode}: stopping", flush=True)
            lines.append(f"# step {name} ended with status {run.returncode}: stopped")
            break
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if run.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
