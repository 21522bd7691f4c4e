#!/usr/bin/env python3
"""GPU box: what a head ensemble costs (include/mmc.h, "head ensembles").

    python tools/ensemble_throughput.py [--blocks 7] [--parent-lib PATH] [--out profiles/ensemble.txt] [--commit ID]

Rewrites the cost section of ``--out`` (everything from the line "# 3. cost ..." on) and keeps what stands in front of it.

Eight heads of the production shape (1280 -> 500 -> 300 -> 100 -> 108, random weights, Platt a in [-3, -0.5], b in [-1, 1]).
Every candidate is warmed up, then timed in alternating blocks between two device events on one stream; the figure is the
median block (min .. max).

(a) mmc_ensemble_topk (k = 3, stats and votes on, device in and out) against what a user composes without it: eight
    mmc_head_predict calls into the slices of one [8][N][108] device tensor, torch.mean over the members, torch.topk.  N = 200 000
    resident rows and N = 1024.  The verdict per size: the ensemble's median at or below the baseline's, or inside the baseline's
    own min .. max.
(b) PointClassifier.classify_images on 16 images of 1500x2000 with 25 points, k = 3, batch_patches 1024: one of the eight heads
    against the eight-head ensemble, host clock, labels on the host at the end of every call, ms per image and the ratio.
(c) mmc_head_topk on the 200 000 rows with this library and with the parent commit's (``--parent-lib``: a libmermaid_mi355.so
    built from the parent commit), alternating blocks in one process; the verdict: this commit's median inside the parent's spread
    or below it.  Without ``--parent-lib`` the part is reported as not measured.
"""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

M, DIMS, K_TOP = 8, (1280, 500, 300, 100, 108), 3
SIZES = ((200000, 5), (1024, 200))            # rows, calls per block
N_IMAGES, POINTS = 16, 25
COST_MARK = "# 3. cost (tools/ensemble_throughput.py)"


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def fmt(v, unit):
    return f"{statistics.median(v):9.3f} {unit}  ({min(v):.3f} .. {max(v):.3f})"


def verdict(new, base):
    mn, mb = statistics.median(new), statistics.median(base)
    if mn <= mb:
        return f"at or below the baseline's median ({mb / mn:.2f}x)"
    if mn <= max(base):
        return f"above the baseline's median by {100 * (mn / mb - 1):.1f} % but inside its min .. max"
    return f"LOSES: above the baseline's median by {100 * (mn / mb - 1):.1f} % and outside its min .. max"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--image-reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ensemble.txt"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks must be at least 5 (the figure is a median of timed blocks)")
    import torch
    if not torch.cuda.is_available():
        sys.exit("ensemble_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import CalibratedMLP, HeadEnsemble, PointClassifier, _lib
    from mermaid_classifier_amd.backbone import Backbone
    from mermaid_classifier_amd.synthetic import synthetic_state_dict

    lib = _lib.lib()
    rng = np.random.default_rng(0)
    K = DIMS[-1]
    members = []
    for _ in range(M):
        W = [rng.normal(0, (2.0 / DIMS[i]) ** 0.5, (DIMS[i + 1], DIMS[i])).astype(np.float32) for i in range(len(DIMS) - 1)]
        b = [rng.normal(0, 0.1, DIMS[i + 1]).astype(np.float32) for i in range(len(DIMS) - 1)]
        members.append(CalibratedMLP(W, b, [f"c{i}" for i in range(K)], rng.uniform(-3, -0.5, K), rng.uniform(-1, 1, K)))
    ens = HeadEnsemble(members)
    h = ens._handle()
    heads = ens._heads
    stream = int(torch.cuda.current_stream(0).cuda_stream)

    def timed(cands, reps):
        for _, fn in cands:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in cands}
        for _ in range(args.blocks):
            for name, fn in cands:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b) / reps)       # milliseconds per call
        return ms

    lines = [
        "# " + " ".join(["python", "tools/ensemble_throughput.py"] + sys.argv[1:]),
        f"# commit {args.commit or commit_id()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"# {M} heads {' -> '.join(map(str, DIMS))}; {args.blocks} alternating blocks per candidate between device events; median block (min .. max)",
    ]
    feats_big = None
    for n, reps in SIZES:
        feats = torch.from_numpy(rng.normal(0.3, 0.6, (n, DIMS[0])).astype(np.float32)).cuda()
        if feats_big is None:
            feats_big = feats
        idx = torch.empty((n, K_TOP), dtype=torch.int32, device="cuda")
        sc = torch.empty((n, K_TOP), dtype=torch.float32, device="cuda")
        stats = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        votes = torch.empty((n,), dtype=torch.int32, device="cuda")
        per = torch.empty((M, n, K), dtype=torch.float32, device="cuda")

        def new():
            _lib.check(lib.mmc_ensemble_topk(h, feats.data_ptr(), n, 1, K_TOP, idx.data_ptr(), sc.data_ptr(), None, stats.data_ptr(),
                                             votes.data_ptr(), 0, stream))

        def composed():
            for j, hd in enumerate(heads):
                _lib.check(lib.mmc_head_predict(hd._h, feats.data_ptr(), n, per[j].data_ptr(), None, 0, stream))
            return torch.topk(per.mean(0), K_TOP, dim=1)

        ms = timed([("mmc_ensemble_topk", new), ("composed baseline", composed)], reps)
        # same answer at the size that is timed (the composed mean is torch's reduction: compare the best class where it is decided)
        new()
        ci = composed()[1]
        torch.cuda.synchronize()
        agree = float((ci[:, 0] == idx[:, 0].long()).float().mean())
        lines.append(f"# (a) N = {n} resident rows, k = {K_TOP}, stats and votes on; {reps} calls per block; ms per call; best class equal to the "
                     f"composed route's on {100 * agree:.3f} % of the rows")
        for name in ms:
            lines.append(f"{name:20s} {fmt(ms[name], 'ms/call')}")
        lines.append(f"verdict N = {n}: mmc_ensemble_topk is {verdict(ms['mmc_ensemble_topk'], ms['composed baseline'])}")
        del per

    # (b)
    g = ROOT / "tests" / "golden"
    bb = Backbone(synthetic_state_dict(seed=0, bn_stats=dict(np.load(g / "synth_bn_stats.npz"))), device=0, max_batch=256)
    images = [rng.integers(0, 256, (1500, 2000, 3), dtype=np.uint8) for _ in range(N_IMAGES)]
    rowcols = [[(int(r), int(c)) for r, c in zip(rng.integers(0, 1500, POINTS), rng.integers(0, 2000, POINTS))] for _ in range(N_IMAGES)]
    routes = [("single head", PointClassifier(bb, members[0].predictor(), batch_patches=1024)),
              ("8-head ensemble", PointClassifier(bb, ens, batch_patches=1024))]
    for _, pc in routes:
        for _ in range(3):
            pc.classify_images(images, rowcols, K_TOP)
    host = {name: [] for name, _ in routes}
    for _ in range(args.blocks):
        for name, pc in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.image_reps):
                pc.classify_images(images, rowcols, K_TOP)       # returns with the labels on the host
            host[name].append((time.perf_counter() - t0) * 1e3 / (args.image_reps * N_IMAGES))
    lines.append(f"# (b) classify_images, {N_IMAGES} images of 1500x2000 with {POINTS} points, k = {K_TOP}, batch_patches 1024; {args.blocks} alternating "
                 f"blocks of {args.image_reps} calls, host clock, labels on the host at the end of every call; ms per image")
    for name in host:
        lines.append(f"{name:20s} {fmt(host[name], 'ms/image')}")
    lines.append(f"ratio 8-head ensemble / single head = {statistics.median(host['8-head ensemble']) / statistics.median(host['single head']):.3f}")

    # (c)
    n, reps = SIZES[0]
    if args.parent_lib:
        parent = C.CDLL(str(Path(args.parent_lib).resolve()))
        fp, vp = C.POINTER(C.c_float), C.c_void_p
        parent.mmc_head_create.argtypes = [C.POINTER(fp), C.POINTER(fp), C.POINTER(C.c_int), C.c_int, fp, fp, C.c_int, C.c_int, C.POINTER(vp)]
        parent.mmc_head_topk.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp, vp, C.c_uint, vp]
        parent.mmc_head_destroy.argtypes = [vp]
        parent.mmc_head_destroy.restype = None
        p = members[0].head_params()
        nl = len(p.weights)
        Wp = (fp * nl)(*[w.ctypes.data_as(fp) for w in p.weights])
        Bp = (fp * nl)(*[v.ctypes.data_as(fp) for v in p.biases])
        dims = (C.c_int * (nl + 1))(*p.dims)
        ph = vp()
        if parent.mmc_head_create(Wp, Bp, dims, nl, p.a.ctypes.data_as(fp), p.b.ctypes.data_as(fp), K, 0, C.byref(ph)) != 0:
            sys.exit("the parent library could not create a head")
        out = {w: (torch.empty((n, K_TOP), dtype=torch.int32, device="cuda"), torch.empty((n, K_TOP), dtype=torch.float32, device="cuda"))
               for w in ("parent", "this commit")}

        def run(which, handle, w):
            i, s = out[w]
            return lambda: _lib.check(which.mmc_head_topk(handle, feats_big.data_ptr(), n, K_TOP, i.data_ptr(), s.data_ptr(), None, 0, stream))
        ms = timed([("parent", run(parent, ph, "parent")), ("this commit", run(lib, heads[0]._h, "this commit"))], reps)
        torch.cuda.synchronize()
        same = bool(torch.equal(out["parent"][0], out["this commit"][0]) and torch.equal(out["parent"][1].view(torch.int32), out["this commit"][1].view(torch.int32)))
        lines.append(f"# (c) mmc_head_topk, one head, N = {n} resident rows, k = {K_TOP}; {reps} calls per block; ms per call; outputs bit-equal: {same}")
        for name in ms:
            lines.append(f"{name:20s} {fmt(ms[name], 'ms/call')}")
        lines.append(f"verdict: this commit is {verdict(ms['this commit'], ms['parent'])}")
        parent.mmc_head_destroy(ph)
    else:
        lines.append("# (c) mmc_head_topk against the parent commit's library: not measured (no --parent-lib)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    # profiles/ensemble.txt holds the resource usage and the error ratios in front: only the cost section is rewritten
    kept = out_path.read_text().split(COST_MARK)[0] if out_path.is_file() else ""
    out_path.write_text(kept + COST_MARK + "\n" + text)


if __name__ == "__main__":
    main()
