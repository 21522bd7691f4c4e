#!/usr/bin/env python3
"""GPU box: what patch views cost (include/mmc.h, "patch views").

    python tools/views_throughput.py [--blocks 7] [--reps 200] [--image-reps 20] [--out profiles/views.txt] [--commit ID]

Part 1, the device cut.  1024 device-resident points on a device-resident 2000x3000 image, cut by mmc_crop_patches and by
mmc_crop_patches_views at views 0, 1, 2, 4, 8 and 9 (all points at the same view), beside Backbone.extract on the 1024 patches
just cut (max_batch 256, the benchmark's pass).  Every candidate is warmed up, then timed in alternating blocks of `reps` calls
between two device events on one stream; the figure is the median block, per patch.  Best case for the cut: the same patch
buffer is rewritten from the same image throughout, and both fit the last-level cache.  The host cut is not measured.
The condition: the pipeline cuts on the copy stream under the backbone pass, so it is bound by the slower of the two, and every
view's cut must cost less per patch than the backbone spends per patch in this visit.  The tool exits non-zero otherwise.

Part 2, images -> labels.  PointClassifier.classify_images on 25-point images (16 images of 1500x2000, head108, k = 3) at
views=(0,) and at all 8 orientations, in alternating blocks of `image-reps` calls timed with the host clock, every call ending with
the labels on the host; median block, per image.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N, VIEWS, H, W = 1024, (0, 1, 2, 4, 8, 9), 2000, 3000
N_IMAGES, POINTS, K_TOP = 16, 25, 3


def commit_id():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--image-reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "views.txt"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks must be at least 5 (the figure is a median of timed blocks)")
    import torch
    if not torch.cuda.is_available():
        sys.exit("views_throughput.py measures on the GPU: no HIP device visible")
    from mermaid_classifier_amd import ALL_ORIENTATIONS, PointClassifier, _lib, load_predictor
    from mermaid_classifier_amd.backbone import Backbone
    from mermaid_classifier_amd.synthetic import synthetic_state_dict

    lib = _lib.lib()
    g = ROOT / "tests" / "golden"
    rng = np.random.default_rng(0)
    bb = Backbone(synthetic_state_dict(seed=0, bn_stats=dict(np.load(g / "synth_bn_stats.npz"))), device=0, max_batch=256)
    image = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    rc = torch.from_numpy(np.stack([rng.integers(0, H, N), rng.integers(0, W, N)], axis=1).astype(np.int32)).cuda()
    codes = {v: torch.full((N,), v, dtype=torch.uint8, device="cuda") for v in VIEWS}
    patches = torch.empty((N, 224, 224, 3), dtype=torch.uint8, device="cuda")
    feats = torch.empty((N, bb.feature_dim), dtype=torch.float32, device="cuda")
    stream = int(torch.cuda.current_stream(0).cuda_stream)

    def plain():
        _lib.check(lib.mmc_crop_patches(image.data_ptr(), H, W, rc.data_ptr(), N, patches.data_ptr(), 0, 0, stream))

    def view(v):
        return lambda: _lib.check(lib.mmc_crop_patches_views(image.data_ptr(), H, W, rc.data_ptr(), N, codes[v].data_ptr(),
                                                             patches.data_ptr(), 0, 0, stream))

    cands = [("mmc_crop_patches", plain)] + [(f"view {v}", view(v)) for v in VIEWS] + [("backbone", lambda: bb.extract(patches, out=feats))]
    for _, fn in cands:                                          # warm-up: code objects, the backbone's graph capture
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in cands}
    for _ in range(args.blocks):
        for name, fn in cands:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            ev[name].append(a.elapsed_time(b) * 1e3 / (args.reps * N))       # microseconds per patch
    med = {k: statistics.median(v) for k, v in ev.items()}
    worst = max(med[f"view {v}"] for v in VIEWS)
    ok = worst < med["backbone"]

    # part 2
    pred = load_predictor(g / "head108" / "model.pt", g / "head108" / "model.json")
    images = [rng.integers(0, 256, (1500, 2000, 3), dtype=np.uint8) for _ in range(N_IMAGES)]
    rowcols = [[(int(r), int(c)) for r, c in zip(rng.integers(0, 1500, POINTS), rng.integers(0, 2000, POINTS))] for _ in range(N_IMAGES)]
    routes = [("views=(0,)", PointClassifier(bb, pred, batch_patches=1024)),
              ("views=0..7", PointClassifier(bb, pred, batch_patches=1024, views=ALL_ORIENTATIONS))]
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
            host[name].append((time.perf_counter() - t0) * 1e3 / (args.image_reps * N_IMAGES))   # milliseconds per image
    hmed = {k: statistics.median(v) for k, v in host.items()}

    lines = [
        "# " + " ".join(["python", "tools/views_throughput.py"] + sys.argv[1:]),
        f"# commit {args.commit or commit_id()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"# part 1: {N} resident points on a resident {H}x{W} image; {args.blocks} alternating blocks of {args.reps} calls per candidate "
        "between device events; median block (min .. max), microseconds per patch",
    ]
    for name, _ in cands:
        lines.append(f"{name:17s} {med[name]:8.4f} us/patch  ({min(ev[name]):.4f} .. {max(ev[name]):.4f})"
                     + ("" if name == "backbone" else f"   = {med[name] / med['backbone']:.3f} of the backbone's time per patch"))
    lines.append(f"condition (every view's cut < backbone per patch): slowest view {worst:.4f} us < {med['backbone']:.4f} us: {ok}")
    lines.append(f"# part 2: classify_images, {N_IMAGES} images of 1500x2000 with {POINTS} points, head108, k = {K_TOP}, batch_patches 1024; "
                 f"{args.blocks} alternating blocks of {args.image_reps} calls, host clock, labels on the host at the end of every call; median (min .. max), ms per image")
    for name, _ in routes:
        lines.append(f"{name:11s} {hmed[name]:8.3f} ms/image  ({min(host[name]):.3f} .. {max(host[name]):.3f})")
    lines.append(f"ratio 8 orientations / single view = {hmed['views=0..7'] / hmed['views=(0,)']:.2f}  (8x the patches)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    if not ok:
        sys.exit("a view's cut costs more per patch than the backbone pass")


if __name__ == "__main__":
    main()
