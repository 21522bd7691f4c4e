#!/usr/bin/env python3
"""GPU box: patches -> top-k labels, the fused route (mmc_classify_patches) against the route a user composes from the pieces.

    python tools/classify_throughput.py [--blocks 7] [--reps 40] [--out profiles/classify_throughput.txt] [--commit ID]

256 device-resident patches, the head108 fixture (K = 108), k = 3 -- one bench.py step with labels at its end.
  fused     PointClassifier.topk_device (mmc_classify_patches: backbone -> head -> calibrate_topk_kernel on one stream), then the
            (256, 3) indices and scores to the host
  composed  Backbone.extract -> (256, 1280) features to the host -> Predictor.predict_proba (features up, (256, 108)
            probabilities down) -> sorted(zip(range(K), row), key=itemgetter(1), reverse=True)[:3] per row on the host
Both run in this process, in alternating timed blocks of `reps` calls after a warm-up of every shape; a block is timed with the
host clock around work that ends in its results being on the host (so the device is idle at both ends).  The figure per route
is the median block; the ratio is composed time / fused time.  The two routes' labels and scores are compared bit for bit first.
"""
import argparse
import statistics
import subprocess
import sys
import time
from operator import itemgetter
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N, K_TOP = 256, 3


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "classify_throughput.txt"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks must be at least 5 (the figure is a median of timed blocks)")
    import torch
    if not torch.cuda.is_available():
        sys.exit("classify_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import PointClassifier, load_predictor
    from mermaid_classifier_amd.backbone import Backbone
    from mermaid_classifier_amd.synthetic import synthetic_state_dict
    from oracle import efficientnet_b0_ref as ref

    g = ROOT / "tests" / "golden"
    bb = Backbone(synthetic_state_dict(seed=0, bn_stats=dict(np.load(g / "synth_bn_stats.npz"))), device=0, max_batch=N)
    pred = load_predictor(g / "head108" / "model.pt", g / "head108" / "model.json")
    pc = PointClassifier(bb, pred)
    patches = torch.from_numpy(np.concatenate([ref.natural_patches(N // 2, seed=7), ref.synthetic_patches(N // 2, seed=42)])).cuda()
    classes = range(len(pred.classes))

    def fused():
        idx, scores = pc.topk_device(patches, K_TOP)
        return idx.cpu().numpy(), scores.cpu().numpy()          # (.cpu() waits for the stream)

    def composed():
        feats = bb.extract(patches).cpu().numpy()
        rows = pred.predict_proba(feats).tolist()
        top = [sorted(zip(classes, row), key=itemgetter(1), reverse=True)[:K_TOP] for row in rows]
        return (np.asarray([[i for i, _ in t] for t in top], np.int32), np.asarray([[s for _, s in t] for t in top], np.float64))

    for _ in range(3):                                          # warm-up: module load, graph capture of both (in, out, n) combinations
        fi, fs = fused()
        ci, cs = composed()
    same = bool(np.array_equal(fi, ci) and np.array_equal(fs.astype(np.float64), cs))
    t = {"fused": [], "composed": []}
    for _ in range(args.blocks):
        for name, fn in (("fused", fused), ("composed", composed)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            t[name].append((time.perf_counter() - t0) / args.reps)
    med = {k: statistics.median(v) for k, v in t.items()}
    ratio = med["composed"] / med["fused"]
    lines = [
        "# " + " ".join(["python", "tools/classify_throughput.py"] + sys.argv[1:]),
        f"# commit {args.commit or commit_id()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"# {N} resident patches, head108 (K = {len(pred.classes)}), k = {K_TOP}; {args.blocks} alternating blocks of {args.reps} calls per route, "
        "host clock, results on the host at the end of every call",
        f"labels and scores of the two routes identical bit for bit: {same}",
    ]
    for name in ("fused", "composed"):
        ms = [x * 1e3 for x in t[name]]
        lines.append(f"{name:9s} median {med[name] * 1e3:7.3f} ms/call = {N / med[name]:9,.0f} patches/s   "
                     f"(blocks min {min(ms):.3f} max {max(ms):.3f} ms/call)")
    lines.append(f"ratio composed / fused = {ratio:.3f}  (>= 1.0: the fused route is not slower)")
    lines.append(f"bytes to the host per call: fused {N * K_TOP * 8:,} (indices + scores); composed {N * 1280 * 4 + N * len(pred.classes) * 4:,} "
                 f"(features + probabilities), plus {N * 1280 * 4:,} back up for the head")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    if not same:
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
