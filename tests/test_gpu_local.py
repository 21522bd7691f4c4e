"""-m gpu: local parity.  Every backbone launch of per-tensor mode (MMC_KEEP_ACTIVATIONS=1) on ITS OWN input as read back
from the device, against the float64 stage reference of ``oracle/local_ref.py``, element by element: |got - ref| <= 2 x the
bound derived from the error model stated at the top of that module.  No RMS, no percentile, no excluded element; the factor
2 is the only margin over the derived worst case.  ``tests/test_gpu_layers.py`` checks what this cannot: the error
accumulated through the chain.  fp16 only: the fp8 project convs have the same check in ``tests/test_gpu_local_fp8.py``.

Per-tensor mode follows ``MMC_TAIL_B11`` and ``MMC_B1_PLANAR``, so the fused schedules run the product's own bodies: all of block 11
inside ``tail7_kernel`` (``b11.tail``, from the block's input, its depthwise output and gate through the kernel's debug taps) and
block 1 on ``mb1_kernel<true>`` / the plane-reading ``thin_proj_kernel``; the test asserts the launch that wrote those tensors.
``b0-fused-split`` switches both off and keeps ``mbconv_a<5,2,...>`` and the interleaved block 1 covered.  What per-tensor mode still
does not run -- the resident single launch of blocks 11-15 + head, the chain, the lanes, graph replay -- is tied to it bit for bit:
``tests/test_gpu_product_route.py`` (features of the product pass == features of per-tensor mode), ``tests/test_gpu_chain.py``.

Measured max |got - ref| / bound per schedule and stage: ``profiles/local_parity.txt``."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FACTOR = 2.0

# schedule -> (architecture, environment at create time)
SCHEDULES = {
    "b0-fused": ("b0", {}),
    "b0-fused-split": ("b0", {"MMC_TAIL_B11": "0", "MMC_B1_PLANAR": "0"}),
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


# the launches that must have written blocks 1 and 11 (a silent fallback to the other route fails the test)
MB1, THIN, TAIL11 = "b0.project+b1.mbconv|mb1", "b1.project|thin_proj", "b11.tail|tail7"
ROUTE = {
    "b0-fused": {"b1.dw": MB1 + "<planar>", "b1.out": THIN + "<planar>", "b11.dw": TAIL11, "b11.gate": TAIL11, "b11.out": TAIL11},
    "b0-fused-split": {"b1.dw": MB1, "b1.out": THIN, "b11.dw": "b11.mbconv|mbconv_a<5,2,", "b11.gate": TAIL11, "b11.out": TAIL11},
}
ROUTE["b0-fused-mfma-dw"] = ROUTE["b0-fused"]
# b0-fused-split against b0-fused.  Blocks 1 and 11 run other launches: every stage of theirs takes its reference.  Blocks 0 and
# 2..10 run the same launches, and block 1's planes hold the bits of its interleaved form (mb1_kernel<true> only moves the store,
# thin_proj_kernel reads plane ks in k-step ks), so their inputs are the same bits: no reference, the output must equal b0-fused's bit
# for bit.  Blocks 12..15 and the features run the same launches on whatever block 11 gave them: decided by the bits at run time.
SPLIT_REFERENCED = {f"b{i}.{t}" for i in (1, 11) for t in ("dw", "gate", "out")}
SPLIT_SHARED = {"b0.dw", "b0.gate"} | {f"b{i}.{t}" for i in range(2, 11) for t in ("dw", "gate", "out")}


def _block_writers(block, stages, launches):
    """The launches that wrote block ``block``'s tensors, stage by stage.  A stage's launch alone does not say it all: the gate's pool
    sums come from the depthwise launch, and ``b11.tail`` is one entry for two argument sets (from the block's input, or from the
    depthwise output of ``b11.mbconv``)."""
    return [_launch_of(st, launches) for st in stages if st.block == block]


def _device_run(schedule, synth_sd, synth_sd_b4, checkpoint_path):
    """One handle of a schedule in per-tensor mode, one extract of the three parity patches: (kept tensors, profile entries)."""
    import torch
    from mermaid_classifier_amd import weights
    from mermaid_classifier_amd.backbone import Backbone
    from oracle import local_ref as lr

    arch, env = SCHEDULES[schedule]
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
    return kept, launches


@pytest.fixture(scope="module")
def fused_run(synth_sd, synth_sd_b4, checkpoint_path):
    """b0-fused's device run, shared by its own check and by b0-fused-split's comparison."""
    return _device_run("b0-fused", synth_sd, synth_sd_b4, checkpoint_path)


@pytest.fixture(scope="module", params=list(SCHEDULES))
def local(request, fused_run, synth_sd, synth_sd_b4, checkpoint_path):
    """One handle per schedule, one extract of the three parity patches, every kept tensor, every stage's (ref, bound).  A stage of
    b0-fused-split whose block runs the same launches as in b0-fused on bit-identical kept inputs has no (ref, bound): its output
    is held to b0-fused's bits instead (``shared``)."""
    from mermaid_classifier_amd import weights
    from oracle import local_ref as lr

    sched = request.param
    arch, _ = SCHEDULES[sched]
    sd_t = synth_sd if arch == "b0" else synth_sd_b4
    kept, launches = fused_run if sched == "b0-fused" else _device_run(sched, synth_sd, synth_sd_b4, checkpoint_path)
    A = weights.get_arch(arch)
    sd = {k: np.asarray(v.numpy(), np.float64) for k, v in sd_t.items() if k in weights.expected_shapes(A)}
    W = lr.Weights(weights.fold(sd, A), A)
    stages = lr.plan(arch, [k for k in kept if k != "patches"])
    results, shared = [], []
    for st in stages:
        if sched == "b0-fused-split":
            base_kept, base_launches = fused_run
            same_launches = (_block_writers(st.block, stages, launches) == _block_writers(st.block, stages, base_launches)
                             and _launch_of(st, launches) == _launch_of(st, base_launches))
            if same_launches and all(
                    nm in base_kept and np.array_equal(kept[nm], base_kept[nm]) for nm in st.inputs):
                shared.append((st, _launch_of(st, launches), np.array_equal(kept[st.name], base_kept[st.name])))
                continue
        ref, bound = lr.run_stage(W, st, kept.__getitem__)
        results.append((st, _launch_of(st, launches), kept[st.name], ref, bound))
    return {"schedule": sched, "arch": arch, "A": A, "kept": kept, "results": results, "shared": shared}


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
    kinds = [st.kind for st, *_ in local["results"]] + [st.kind for st, *_ in local["shared"]]
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
    for st, launch, equal in local["shared"]:
        lines.append(f"{sched:18s} {st.name:12s} {st.kind:9s} {launch:40s} same launches and input bits as b0-fused: output bits "
                     f"{'equal' if equal else 'DIFFER'}")
        if not equal:
            failures.append(f"stage {st.name} ({st.kind}), launch {launch}: same launches on the same input bits as b0-fused, other output bits")
    print("\n".join(lines))
    out_dir = os.environ.get("MMC_LOCAL_PARITY_OUT")      # tools: keep the table (profiles/local_parity.txt)
    if out_dir:
        with open(os.path.join(out_dir, f"local_parity_{sched}.txt"), "w") as f:
            f.write("\n".join(lines + failures) + "\n")
    # the launches that wrote blocks 1 and 11, and which stages took a reference
    written_by = {st.name: launch for st, launch, *_ in local["results"] + local["shared"]}
    for name, entry in ROUTE.get(sched, {}).items():
        assert written_by[name] == entry or (entry.endswith(",") and written_by[name].startswith(entry)), \
            f"{sched}: {name} was written by {written_by[name]}, expected {entry}"
    if sched == "b0-fused-split":
        referenced, same_bits = {st.name for st, *_ in local["results"]}, {st.name for st, *_ in local["shared"]}
        assert SPLIT_REFERENCED <= referenced and SPLIT_SHARED <= same_bits, \
            f"referenced {sorted(referenced)}, shared with b0-fused {sorted(same_bits)}"
    else:
        assert not local["shared"]
    assert not failures, f"{len(failures)} of {len(kinds)} stages exceed {FACTOR:g} x bound or differ from b0-fused\n" + "\n".join(failures)
