"""-m gpu: local parity.  Every backbone launch of per-tensor mode (MMC_KEEP_ACTIVATIONS=1) on ITS OWN input as read back
from the device, against the float64 stage reference of ``oracle/local_ref.py``, element by element: |got - ref| <= 2 x the
bound derived from the error model stated at the top of that module.  No RMS, no percentile, no excluded element; the factor
2 is the only margin over the derived worst case.  ``tests/test_gpu_layers.py`` checks what this cannot: the error
accumulated through the chain.  fp16 only: the fp8 project convs have the same check in ``tests/test_gpu_local_fp8.py``; the
product-only routes per-tensor mode does not run are out of scope.

Measured max |got - ref| / bound per schedule and stage: ``profiles/local_parity.txt``."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FACTOR = 2.0

# schedule -> (architecture, environment at create time)
SCHEDULES = {
    "b0-fused": ("b0", {}),
    "b0-unfused": ("b0", {"MMC_FUSE": "0"}),
    "b0-fused-mfma-dw": ("b0", {"MMC_MID14M": "1", "MMC_MBT4": "1"}),
    "b4": ("b4", {}),
    "b4-unfused": ("b4", {"MMC_FUSE": "0"}),
}


def _launch_of(stage, launches):
    """The ``Backbone.profile`` entry ("name|label") of the launch that wrote a stage's tensor."""
    if stage.kind in ("stem", "expand"):
        keys = [stage.name]
    elif stage.kind == "features":
        keys = ["head"]
    else:
        b = f"b{stage.block}."
        keys = {"gate": [b + "gate", b + "projse", b + "tail"], "out": [b + "project", b + "projse", b + "tail"]}.get(
            stage.kind, [b + "dw", b + "mbconv", b + "tail"])
    for k in keys:
        for entry in launches:
            parts = entry.split("|")[0].split("+")      # "b0.project+b1.mbconv|mb1", "b12.tail|tail7", "head.tail|tail7"
            if k in parts or (k == "head" and parts[0].startswith("head")):
                return entry
    return "?"


@pytest.fixture(scope="module", params=list(SCHEDULES))
def local(request, synth_sd, synth_sd_b4, checkpoint_path):
    """One handle per schedule, one extract of the three parity patches, every kept tensor, every stage's (ref, bound)."""
    import torch
    from mermaid_classifier_amd import weights
    from mermaid_classifier_amd.backbone import Backbone
    from oracle import local_ref as lr

    arch, env = SCHEDULES[request.param]
    sd_t = synth_sd if arch == "b0" else synth_sd_b4
    os.environ["MMC_KEEP_ACTIVATIONS"] = "1"
    os.environ.update(env)
    try:
        if arch == "b0":
            bb = Backbone(str(checkpoint_path), device=0, max_batch=4)
        else:
            bb = Backbone({k: v.numpy() for k, v in sd_t.items()}, device=0, max_batch=4)
    finally:
        os.environ.pop("MMC_KEEP_ACTIVATIONS", None)
        for k in env:
            os.environ.pop(k, None)
    try:
        patches = lr.parity_patches()
        n = len(patches)
        dev = torch.from_numpy(patches).cuda()
        launches = [nm for nm, _ in bb.profile(dev, torch.empty((n, bb.feature_dim), dtype=torch.float32, device="cuda"))]
        feats = bb.extract(patches)
        A = weights.get_arch(arch)
        names = ["stem"] + [f"b{i}.{t}" for i in range(len(A.blocks)) for t in ("expand", "dw", "gate", "out")]
        kept = {"patches": patches, "features": feats}
        for nm in names:
            shape = lr.tensor_shape(arch, nm, n)
            try:
                kept[nm] = bb.read_activation(nm, int(np.prod(shape))).reshape(shape).copy()
            except ValueError:
                pass      # not kept by this schedule; lr.plan and the test decide whether that is allowed
    finally:
        bb.close()
    sd = {k: np.asarray(v.numpy(), np.float64) for k, v in sd_t.items() if k in weights.expected_shapes(A)}
    W = lr.Weights(weights.fold(sd, A), A)
    stages = lr.plan(arch, [k for k in kept if k != "patches"])
    results = []
    for st in stages:
        ref, bound = lr.run_stage(W, st, kept.__getitem__)
        results.append((st, _launch_of(st, launches), kept[st.name], ref, bound))
    return {"schedule": request.param, "arch": arch, "A": A, "kept": kept, "results": results}


def test_every_stage_within_twice_its_bound(local):
    from oracle import local_ref as lr
    A, kept, sched = local["A"], local["kept"], local["schedule"]
    nb = len(A.blocks)
    # coverage: nothing skipped silently
    have = set(kept) - {"patches"}
    always = {"features"} | {f"b{i}.{t}" for i in range(nb) for t in ("dw", "gate", "out")}
    expands = {f"b{i}.expand" for i, b in enumerate(A.blocks) if b[2] != 1}
    if sched.startswith("b0-fused"):
        want = always - {"b0.out"}           # stem and block 0's output live only in LDS / registers
    elif sched.endswith("unfused"):
        want = always | expands | {"stem"}
    else:
        want = always | {"stem"}             # B4: the fused front halves keep no expanded tensor
    assert have == want, f"{sched}: missing {sorted(want - have)}, unexpected {sorted(have - want)}"
    kinds = [st.kind for st, *_ in local["results"]]
    if local["arch"] == "b0":
        assert len(kinds) == (65 if sched == "b0-unfused" else 48)
    else:
        assert len(kinds) == 2 + 3 * nb + (len(expands) if sched == "b4-unfused" else 0)
    lines, failures = [], []
    for st, launch, got, ref, bound in local["results"]:
        assert got.shape == ref.shape == bound.shape and np.isfinite(got).all() and np.isfinite(bound).all(), st.name
        ratio, idx = lr.worst_ratio(got, ref, bound)
        lines.append(f"{sched:18s} {st.name:12s} {st.kind:9s} {launch:40s} max|got-ref|/bound {ratio:6.3f} at {idx}")
        rep = lr.exceed_report(got, ref, bound, FACTOR)
        if rep:
            failures.append(f"stage {st.name} ({st.kind}), launch {launch}: {rep}")
    print("\n".join(lines))
    out_dir = os.environ.get("MMC_LOCAL_PARITY_OUT")      # tools: keep the table (profiles/local_parity.txt)
    if out_dir:
        with open(os.path.join(out_dir, f"local_parity_{sched}.txt"), "w") as f:
            f.write("\n".join(lines + failures) + "\n")
    assert not failures, f"{len(failures)} of {len(kinds)} stages exceed {FACTOR:g} x bound\n" + "\n".join(failures)
