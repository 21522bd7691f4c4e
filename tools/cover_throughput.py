#!/usr/bin/env python3
"""GPU box: what cover estimation costs (include/mmc.h, "cover estimation").

    python tools/cover_throughput.py [--rows 200000] [--blocks 7] [--reps 10] [--out profiles/cover.txt] [--commit ID]

200 000 x 108 resident rows (head108 on seeded device features), once as one source-sized group and once as 25-point groups.
Each layout is measured by a child process of its own under `timeout`; the parent never opens the GPU and starts nothing more after
a step that fails.  Per layout, every candidate is warmed up and then timed in alternating blocks of `reps` calls with the host
clock (every call ends in its own stream synchronisation); the figure is the median block, per call:

    head pass      mmc_head_predict over the rows, device in, device out
    head top-k     mmc_head_topk (k = 4) over the rows, device out: the serving call of the parent commit, for scale
    count pass     mmc_cover_proba on the resident probabilities with iters = 0 and no top-k: uploads, count kernel, tables back
    EM iteration   (mmc_cover_proba with iters = 20  -  the same with iters = 0) / 20
    adapted top-k  (mmc_cover_proba with iters = 0, k = 4, device out  -  the same without top-k)
    whole call     mmc_head_cover (iters = 20, k = 4, device in, device top-k out): head pass + stage

and one iteration's bytes (rows x K x 4) over its time.  The one condition: an EM iteration takes less time than mmc_head_predict
over the same rows in the same run (which reads twelve times the bytes and does all the arithmetic); the tool exits non-zero
otherwise.  All other numbers are recorded, not gated.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

K_TOP, EM_ITERS, STEP_SECONDS = 4, 20, 240
LAYOUTS = ("one group", "25-point groups")


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def step(layout: str, rows: int, blocks: int, reps: int) -> dict:
    """One layout, in this process: -> {candidate: [seconds per call, one per block]} plus device and shape facts."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("cover_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import _lib, load_predictor
    lib = _lib.lib()
    g = ROOT / "tests" / "golden"
    head = load_predictor(g / "head108" / "model.pt", g / "head108" / "model.json")._head
    K = head.n_classes
    torch.manual_seed(0)
    feats = torch.randn((rows, head.input_dim), dtype=torch.float32, device="cuda") * 0.6 + 0.3
    proba = torch.empty((rows, K), dtype=torch.float32, device="cuda")
    idx = torch.empty((rows, K_TOP), dtype=torch.int32, device="cuda")
    scores = torch.empty((rows, K_TOP), dtype=torch.float32, device="cuda")
    sizes = [rows] if layout == LAYOUTS[0] else [25] * (rows // 25) + ([rows % 25] if rows % 25 else [])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    G = len(sizes)
    tp = np.random.default_rng(0).dirichlet(np.full(K, 2.0))
    tables = [np.zeros((G, K), np.int64), np.zeros((G, K), np.int64), np.zeros(G, np.int64), np.zeros((G, K), np.float64)]
    tptr = [t.ctypes.data for t in tables]
    stream = int(torch.cuda.current_stream(0).cuda_stream)

    def predict():
        _lib.check(lib.mmc_head_predict(head._h, feats.data_ptr(), rows, proba.data_ptr(), None, 0, stream))
        torch.cuda.synchronize()

    def topk():
        _lib.check(lib.mmc_head_topk(head._h, feats.data_ptr(), rows, K_TOP, idx.data_ptr(), scores.data_ptr(), None, 0, stream))
        torch.cuda.synchronize()

    def stage(iters, k):
        return lambda: _lib.check(lib.mmc_cover_proba(proba.data_ptr(), rows, K, off.ctypes.data, G, tp.ctypes.data, 1.0, iters, *tptr, k,
                                                      idx.data_ptr() if k else None, scores.data_ptr() if k else None, 0, 0, stream))

    def whole():
        _lib.check(lib.mmc_head_cover(head._h, feats.data_ptr(), rows, 1, off.ctypes.data, G, tp.ctypes.data, 1.0, EM_ITERS, *tptr, K_TOP,
                                      idx.data_ptr(), scores.data_ptr(), 0, stream))

    cands = [("predict", predict), ("topk", topk), ("stage_0", stage(0, 0)), ("stage_em", stage(EM_ITERS, 0)), ("stage_topk", stage(0, K_TOP)),
             ("whole", whole)]
    for _, fn in cands:
        for _ in range(2):
            fn()
    times = {name: [] for name, _ in cands}
    for _ in range(blocks):
        for name, fn in cands:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            times[name].append((time.perf_counter() - t0) / reps)
    return dict(layout=layout, rows=rows, K=K, groups=G, device=torch.cuda.get_device_name(0), torch=torch.__version__, times=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cover.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks must be at least 5 (the figure is a median of timed blocks)")
    if args.step is not None:
        print("RESULT " + json.dumps(step(args.step, args.rows, args.blocks, args.reps)), flush=True)
        return
    results = []
    for layout in LAYOUTS:                                       # one child per layout, each under its own time limit
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, str(Path(__file__).resolve()), "--step", layout, "--rows", str(args.rows),
               "--blocks", str(args.blocks), "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"step {layout!r} ended with status {p.returncode}: nothing more is started")
        results.append(json.loads(next(line for line in p.stdout.splitlines() if line.startswith("RESULT "))[7:]))
    ms = 1e3
    lines = ["# " + " ".join(["python", "tools/cover_throughput.py"] + sys.argv[1:]),
             f"# commit {args.commit or commit_id()}; {results[0]['device']}; torch {results[0]['torch']}",
             f"# {args.rows} x {results[0]['K']} resident rows (head108); per layout {args.blocks} alternating blocks of {args.reps} calls per "
             "candidate, host clock around calls that end in a stream synchronisation; median block (min .. max), milliseconds per call"]
    ok = True
    for r in results:
        t = r["times"]
        med = {k: statistics.median(v) for k, v in t.items()}
        em = (med["stage_em"] - med["stage_0"]) / EM_ITERS
        tk = med["stage_topk"] - med["stage_0"]
        nbytes = r["rows"] * r["K"] * 4
        good = em < med["predict"]
        ok = ok and good
        lines.append(f"## {r['layout']}: {r['groups']} groups")
        for name, label in (("predict", "head pass (mmc_head_predict)"), ("topk", f"mmc_head_topk, k = {K_TOP}"),
                            ("stage_0", "count pass (stage, iters 0, no top-k)"), ("stage_em", f"stage, iters {EM_ITERS}, no top-k"),
                            ("stage_topk", f"stage, iters 0, top-{K_TOP}"), ("whole", f"mmc_head_cover, iters {EM_ITERS}, top-{K_TOP}")):
            lines.append(f"{label:42s} {med[name] * ms:9.4f} ms  ({min(t[name]) * ms:.4f} .. {max(t[name]) * ms:.4f})")
        lines.append(f"{'one EM iteration (difference / ' + str(EM_ITERS) + ')':42s} {em * ms:9.4f} ms   {nbytes / em / 1e9:8.1f} GB/s of rows x K x 4 bytes")
        lines.append(f"{'adapted top-k (difference)':42s} {tk * ms:9.4f} ms")
        lines.append(f"condition (one EM iteration < mmc_head_predict): {em * ms:.4f} ms < {med['predict'] * ms:.4f} ms: {good}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    if not ok:
        sys.exit("an EM iteration costs more than mmc_head_predict over the same rows")


if __name__ == "__main__":
    main()
