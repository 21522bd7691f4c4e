"""Wall time of logit calibration (mmc_logitcal_*) at the production shape, beside torch fp64 doing the same sums on the same card,
and the error / bound figures the GPU tests print.

    python tools/logit_scaling_cost.py [--rows 200000] [--classes 108] [--dim 1280] [--out profiles/logit_scaling.txt]

Four steps, each in a child process of its own under `timeout` (the parent stops at the first child that fails):
  store   add_set of --rows resident rows through a production head (1280 -> 500 -> 300 -> 100 -> K), then one pass of sums with and
          without the Hessian
  fit     each mode's whole fit on stored logits with a known miscalibration, with its trial count
  torch   the same sums (loss, gradient, D, sum v v^T) in torch float64 on the card: a yardstick that is recorded, not gated
  tests   tests/test_gpu_logit_scaling.py with its output shown: the worst error / bound ratios and the parameter gap to the checker's
          optimum
Every timed call ends in a synchronisation; the host clock is around it; the line gives the median and the spread after one warm-up.
None of these times is gated anywhere.
"""

from __future__ import annotations

import argparse
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

REPEATS = 5
STEPS = {"store": 300, "fit": 300, "torch": 300, "tests": 300}   # seconds allowed per child


def spread(times):
    return f"median {statistics.median(times) * 1e3:.2f} ms (min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}, {len(times)} repeats after 1 warm-up)"


def timed(call, repeats=REPEATS):
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


def miscalibrated_logits(n: int, K: int, seed: int = 0):
    """tests/logit_scaling_checker.fixture at any size: an over-confident head with per-class gains and offsets."""
    sys.path.insert(0, str(ROOT / "tests"))
    import logit_scaling_checker as ck
    return ck.fixture(n, K, seed=seed)


def step_store(n: int, K: int, dim: int) -> None:
    from mermaid_classifier_amd import FeatureSet
    from mermaid_classifier_amd.logit_scaling import _LogitCalibrator
    from mermaid_classifier_amd.torch_classifier import TorchMLPClassifier
    rng = np.random.default_rng(0)
    centers = rng.normal(0.0, 0.08, size=(K, dim)).astype(np.float32)
    fs = FeatureSet(dim, np.arange(K), reserve=n)
    for first in range(0, n, 20000):
        m = min(20000, n - first)
        y = rng.integers(0, K, m)
        fs.append(centers[y] + rng.normal(0.0, 1.0, size=(m, dim)).astype(np.float32), y)
    clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), random_state=0)
    X, y = fs.read(0, 6000)
    clf.partial_fit(X, y, classes=np.arange(K).tolist())

    def add():
        cal = _LogitCalibrator(K)
        cal.add_set(clf, fs)
        cal.close()
    print(f"mmc_logitcal_add_set  {n} x {dim} -> {K} logits (forward + store, handle created and destroyed): {spread(timed(add))}", flush=True)
    cal = _LogitCalibrator(K)
    cal.add_set(clf, fs)
    a, c = np.ones(K), np.zeros(K)
    t_h = timed(lambda: cal.stats(a, c, hess=True))
    t_g = timed(lambda: cal.stats(a, c, hess=False))
    flop = 2.0 * n * (2 * K) * (2 * K) / 2
    print(f"mmc_logitcal_stats    {n} x {K} with the Hessian: {spread(t_h)}; {flop / statistics.median(t_h) / 1e12:.2f} TFLOP/s fp64 on the "
          f"upper triangle", flush=True)
    print(f"mmc_logitcal_stats    {n} x {K} without the Hessian: {spread(t_g)}", flush=True)
    cal.close()


def step_fit(n: int, K: int, dim: int) -> None:
    from mermaid_classifier_amd.logit_scaling import _LogitCalibrator
    z, y = miscalibrated_logits(n, K)
    cal = _LogitCalibrator(K)
    for first in range(0, n, 50000):
        cal.add_logits(z[first:first + 50000], y[first:first + 50000])
    for kind in ("temperature", "bias", "vector"):
        res = cal.fit(kind)
        t = timed(lambda: cal.fit(kind), 3)
        print(f"mmc_logitcal_fit      {n} x {K} {kind}: {spread(t)}; {res.trials} trial points, converged={res.converged}, mean nll "
              f"{res.nll_before:.6f} -> {res.nll_after:.6f}", flush=True)
    cal.close()


def step_torch(n: int, K: int, dim: int) -> None:
    import torch
    z, y = miscalibrated_logits(n, K)
    zt = torch.from_numpy(z).cuda()
    yt = torch.from_numpy(y.astype(np.int64)).cuda()
    a = torch.ones(K, dtype=torch.float64, device="cuda")
    c = torch.zeros(K, dtype=torch.float64, device="cuda")

    def sums(hess: bool):
        zd = zt.double()
        u = a * zd + c
        lse = torch.logsumexp(u, dim=1)
        p = torch.exp(u - lse[:, None])
        nll = (lse - u.gather(1, yt[:, None])[:, 0]).sum()
        r = p.clone()
        r[torch.arange(n, device="cuda"), yt] -= 1.0
        out = [nll, (zd * r).sum(0), r.sum(0)]
        if hess:
            v = torch.cat([zd * p, p], dim=1)
            out += [v.T @ v, (zd * zd * p).sum(0), (zd * p).sum(0), p.sum(0)]
        torch.cuda.synchronize()
        return out
    print(f"torch float64         {n} x {K} the same sums with the Hessian: {spread(timed(lambda: sums(True)))}", flush=True)
    print(f"torch float64         {n} x {K} the same sums without the Hessian: {spread(timed(lambda: sums(False)))}", flush=True)


def step_tests() -> int:
    run = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_logit_scaling.py"), "-q", "-s", "-p", "no:cacheprovider"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(ROOT))
    found = re.findall(r"logit_scaling: (.*)", run.stdout)
    worst = {"nll": 0.0, "grad": 0.0, "hess": 0.0}
    for ln in found:
        m = re.match(r"stats .*error/bound nll (\S+) grad (\S+) hess (\S+)", ln)
        if m:
            for key, val in zip(worst, m.groups()):
                worst[key] = max(worst[key], float(val))
        else:
            print(ln)
    print(f"stats, worst error / bound over {sum(ln.startswith('stats') for ln in found)} cases: nll {worst['nll']:.3g}, grad {worst['grad']:.3g}, "
          f"hess {worst['hess']:.3g} (gate: 1)")
    print(run.stdout.strip().splitlines()[-1], flush=True)
    return run.returncode


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--classes", type=int, default=108)
    ap.add_argument("--dim", type=int, default=1280)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step == "tests":
        return step_tests()
    if args.step:
        {"store": step_store, "fit": step_fit, "torch": step_torch}[args.step](args.rows, args.classes, args.dim)
        return 0
    lines = [f"# python tools/logit_scaling_cost.py --rows {args.rows} --classes {args.classes} --dim {args.dim}",
             "# each step in its own process; host clock around calls that end in a synchronisation; nothing here is gated"]
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--step", name, "--rows", str(args.rows),
               "--classes", str(args.classes), "--dim", str(args.dim)]
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
