"""Wall time of mmc_featureset_knn (cosine, k = 10) at production shapes, beside the same search done with torch on the same card:
chunked fp32 matmul + topk, which writes and re-reads every chunk of the score matrix.

    python tools/knn_cost.py [--base 200000] [--queries 20000] [--dim 1280] [--k 10] [--out profiles/knn_cost.txt]

Two shapes, each in a child process of its own under `timeout` (the parent stops at the first child that fails):
  cross   --queries x --base rows of two resident sets
  self    the --base-row self-search with the row's own image excluded (4 rows per image)
The rows are made on the device (seeded, non-negative, 64 correlated directions plus noise) and appended to resident sets.  Each side
is warmed up once at the full shape, then timed REPEATS times with the host clock around calls that end in a synchronisation; the
line gives the median and the spread.  The torch figure is a yardstick that is recorded, not gated.
"""

from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

K_CLASSES = 40
FP32_MATRIX_ROOF = 157e12   # FLOP/s, exact-f32 MFMA peak of an MI355X
REPEATS = 5
TORCH_CHUNK = 4096          # query rows per matmul: a 4096 x 200000 fp32 score block is 3.3 GB
STEPS = {"cross": 300, "self": 540}   # seconds allowed per child


def device_rows(n: int, dim: int, seed: int):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    mix = torch.randn(64, dim, generator=g, device="cuda")
    base = 3 + 6 * torch.rand(dim, generator=g, device="cuda")
    X = torch.empty(n, dim, device="cuda")
    for first in range(0, n, 20000):
        m = min(20000, n - first)
        X[first:first + m] = (base + torch.randn(m, 64, generator=g, device="cuda") @ mix / 8
                              + 0.3 * torch.randn(m, dim, generator=g, device="cuda")).clamp_(min=0)
    return X


def resident(X, seed: int):
    from mermaid_classifier_amd import FeatureSet
    y = np.random.default_rng(seed).integers(0, K_CLASSES, X.shape[0])
    return FeatureSet(X.shape[1], np.arange(K_CLASSES), reserve=X.shape[0]).append_device(X, y)


def spread(times):
    return f"median {statistics.median(times) * 1e3:.1f} ms (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}, {len(times)} repeats after 1 warm-up)"


def fused(q, nq, b, nb, k, groups, exclude_self):
    """-> (timed call, index tensor): the raw entry with device outputs and device groups"""
    import torch
    from mermaid_classifier_amd import _lib
    index = torch.empty(nq, k, dtype=torch.int32, device="cuda")
    score = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    flags = _lib.MMC_KNN_EXCLUDE_SELF if exclude_self else 0
    g = None if groups is None else groups.data_ptr()
    torch.cuda.synchronize()

    def call():
        _lib.check(_lib.lib().mmc_featureset_knn(q._handle(), 0, nq, b._handle(), 0, nb, k, _lib.MMC_KNN_COSINE, g, g, index.data_ptr(),
                                                 score.data_ptr(), None, flags, None))
    return call, index


def torch_search(Xq, Xb, k, groups, exclude_self):
    import torch
    index = torch.empty(Xq.shape[0], k, dtype=torch.int64, device="cuda")

    def call():
        qn = Xq / Xq.norm(dim=1, keepdim=True).clamp_min(1e-30)
        bn = Xb / Xb.norm(dim=1, keepdim=True).clamp_min(1e-30)
        for first in range(0, Xq.shape[0], TORCH_CHUNK):
            S = qn[first:first + TORCH_CHUNK] @ bn.T
            if groups is not None:
                S.masked_fill_(groups[first:first + TORCH_CHUNK, None] == groups[None, :], float("-inf"))
            elif exclude_self:
                S.diagonal(offset=first).fill_(float("-inf"))
            index[first:first + TORCH_CHUNK] = torch.topk(S, k, dim=1).indices
        torch.cuda.synchronize()
    return call, index


def timed(call, repeats):
    call()                                     # warm-up at the full shape
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


def step(name: str, nb: int, nq: int, dim: int, k: int) -> None:
    import torch
    torch.backends.cuda.matmul.allow_tf32 = False
    Xb = device_rows(nb, dim, seed=1)
    b = resident(Xb, seed=2)
    if name == "cross":
        Xq = device_rows(nq, dim, seed=3)
        q, groups, exclude = resident(Xq, seed=4), None, False
        what = f"{nq} x {nb} x {dim}, k = {k}, cosine"
    else:
        Xq, q, nq, exclude = Xb, b, nb, True
        groups = (torch.arange(nb, device="cuda") // 4).to(torch.int32)
        what = f"{nb}-row self-search x {dim}, k = {k}, cosine, own image (4 rows) excluded"
    flop = 2.0 * nq * nb * dim
    call, f_index = fused(q, nq, b, nb, k, groups, exclude)
    t = timed(call, REPEATS)
    med = statistics.median(t)
    print(f"mmc_featureset_knn   {what}: {spread(t)}; {flop / med / 1e12:.1f} TFLOP/s = {flop / med / FP32_MATRIX_ROOF:.3f} of the "
          f"157 TF fp32-matrix roof", flush=True)
    call_t, t_index = torch_search(Xq, Xb, k, groups, exclude)
    tt = timed(call_t, 3)
    med_t = statistics.median(tt)
    same = float((f_index.to(torch.int64) == t_index).all(dim=1).float().mean())
    print(f"torch matmul + topk  {what}: {spread(tt)}; {flop / med_t / 1e12:.1f} TFLOP/s; chunks of {TORCH_CHUNK} queries", flush=True)
    print(f"fused / torch time   {med / med_t:.2f}; queries whose {k} indices agree between the two {same:.4f} (torch's fp32 product "
          f"rounds in another order)", flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", type=int, default=200000)
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=1280)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.base, args.queries, args.dim, args.k)
        return 0
    lines = [f"# python tools/knn_cost.py --base {args.base} --queries {args.queries} --dim {args.dim} --k {args.k}",
             "# each shape in its own process; host clock around calls that end in a synchronisation; device inputs and outputs"]
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--step", name, "--base", str(args.base),
               "--queries", str(args.queries), "--dim", str(args.dim), "--k", str(args.k)]
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
