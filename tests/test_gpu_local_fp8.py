"""-m gpu: local parity of the fp8 project convs (``Backbone(..., arch="b4", precision="fp8")``, ``pw_gemm_fp8_kernel``), the
companion of ``tests/test_gpu_local.py``.  Per-tensor mode (MMC_KEEP_ACTIVATIONS=1) on the three parity patches with
max_batch=4: 147 GEMM rows at 7x7 (two full 64-row workgroups and a ragged one, 16-row fragments straddling patches), 588 at
14x14.  Two schedules: ``b4-fp8`` (blocks 22-31: K = 960 / 1632 / 2688, N = 272 / 448) and ``b4-fp8-14`` (MMC_FP8_MAXH=14, blocks
10-31: adds K = 336 / 672 / 960, N = 112 / 160, HW = 196); both with and without a skip.

* the fp8 block set read off ``Backbone.profile`` equals the one the architecture table gives;
* every kept tensor before the first fp8 block is bit-identical to the fp16 handle's (those stages have their references in
  ``test_gpu_local.py``);
* from the first fp8 block to the features every launch is checked on ITS OWN device input, element by element, against the
  float64 stage reference of ``oracle/local_ref.py``: |got - ref| <= 2 x bound, ``out_fp8`` (rule 7: the operand codes replicated
  bit for bit, so the bound holds only fp32 accumulation and the fp16 store) for the fp8 blocks, the fp16 stage references for
  the rest.  No element is excluded;
* at most 1e-4 of an ``out_fp8`` stage's activation operands sit within 4 fp32 ulps of an e4m3 rounding boundary (the only
  operands whose code the bound lets move).

An all-zero pixel row (``mx == 0``) cannot be produced through the backbone's inputs: ``tests/test_local_ref_fp8.py`` covers it
on the CPU emulation only.  ``tests/test_local_ref_fp8.py`` also proves the gate sound and sharp before any GPU run.

Measured max |got - ref| / bound per schedule and stage: ``profiles/local_parity.txt``."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FACTOR = 2.0

# schedule -> (largest output side whose project conv runs on e4m3 operands, environment at create time)
SCHEDULES = {
    "b4-fp8": (7, {}),
    "b4-fp8-14": (14, {"MMC_FP8_MAXH": "14"}),
}


def _capture(sd_t, precision, env):
    """One B4 handle in per-tensor mode, one pass over the three parity patches: (profile entries, every kept tensor)."""
    import torch
    from mermaid_classifier_amd import weights
    from mermaid_classifier_amd.backbone import Backbone
    from oracle import local_ref as lr

    os.environ["MMC_KEEP_ACTIVATIONS"] = "1"
    os.environ.update(env)
    try:
        bb = Backbone({k: v.numpy() for k, v in sd_t.items()}, device=0, max_batch=4, precision=precision)
    finally:
        os.environ.pop("MMC_KEEP_ACTIVATIONS", None)
        for k in env:
            os.environ.pop(k, None)
    try:
        patches = lr.parity_patches()
        n = len(patches)
        dev = torch.from_numpy(patches).cuda()
        launches = [nm for nm, _ in bb.profile(dev, torch.empty((n, bb.feature_dim), dtype=torch.float32, device="cuda"))]
        kept = {"patches": patches, "features": bb.extract(patches)}
        A = weights.get_arch("b4")
        for nm in ["stem"] + [f"b{i}.{t}" for i in range(len(A.blocks)) for t in ("expand", "dw", "gate", "out")]:
            shape = lr.tensor_shape("b4", nm, n)
            try:
                kept[nm] = bb.read_activation(nm, int(np.prod(shape))).reshape(shape).copy()
            except ValueError:
                pass      # not kept by this schedule; lr.plan and the tests decide whether that is allowed
    finally:
        bb.close()
    return launches, kept


def _block_of(name):
    return int(name[1:name.index(".")]) if name[0] == "b" and "." in name else -1


def _launch_of(stage, launches):
    if stage.kind == "features":
        keys = ["head"]
    else:
        b = f"b{stage.block}."
        keys = {"gate": [b + "gate", b + "projse"], "out": [b + "project", b + "projse"], "out_fp8": [b + "project"]}.get(
            stage.kind, [b + "dw", b + "mbconv"])
    for k in keys:
        for entry in launches:
            parts = entry.split("|")[0].split("+")
            if k in parts or (k == "head" and parts[0].startswith("head")):
                return entry
    return "?"


@pytest.fixture(scope="module")
def half(synth_sd_b4):
    """The fp16 B4 handle with the same keep flag: the bits the fp8 flag must not touch."""
    return _capture(synth_sd_b4, "fp16", {})


@pytest.fixture(scope="module", params=list(SCHEDULES))
def local(request, synth_sd_b4):
    from mermaid_classifier_amd import weights
    from oracle import local_ref as lr

    maxh, env = SCHEDULES[request.param]
    launches, kept = _capture(synth_sd_b4, "fp8", env)
    A = weights.get_arch("b4")
    # the expected fp8 blocks, from the architecture table alone: output side <= maxh
    want, h = [], 112
    for i, (k, s, e, cin, cout) in enumerate(A.blocks):
        h = -(-h // s)
        if h <= maxh:
            want.append(i)
    sd = {k: np.asarray(v.numpy(), np.float64) for k, v in synth_sd_b4.items() if k in weights.expected_shapes(A)}
    W = lr.Weights(weights.fold(sd, A), A)
    first = want[0]
    stages = [st for st in lr.plan("b4", [k for k in kept if k != "patches"], fp8_blocks=set(want))
              if st.kind == "features" or st.block >= first]
    results, info = [], {}
    for st in stages:
        ref, bound = lr.run_stage(W, st, kept.__getitem__, info)
        results.append((st, _launch_of(st, launches), kept[st.name], ref, bound))
    return {"schedule": request.param, "A": A, "launches": launches, "kept": kept, "want": want, "results": results, "info": info}


def test_fp8_block_set(local, half):
    nb = len(local["A"].blocks)
    got = [e for e in local["launches"] if "fp8" in e]
    assert got == [f"b{i}.project|pw_gemm_fp8" for i in local["want"]], (local["schedule"], got)
    assert local["want"] == list(range({"b4-fp8": 22, "b4-fp8-14": 10}[local["schedule"]], nb))
    assert not [e for e in half[0] if "fp8" in e]
    # the shapes this file is about are all live
    K = {local["A"].blocks[i][2] * local["A"].blocks[i][3] for i in local["want"]}
    N = {local["A"].blocks[i][4] for i in local["want"]}
    assert (K, N) == ({"b4-fp8": ({960, 1632, 2688}, {272, 448}),
                       "b4-fp8-14": ({336, 672, 960, 1632, 2688}, {112, 160, 272, 448})}[local["schedule"]])


def test_tensors_before_the_first_fp8_block_are_the_fp16_handle_s(local, half):
    kept, first = local["kept"], local["want"][0]
    assert set(kept) == set(half[1])
    before = [nm for nm in kept if nm == "stem" or 0 <= _block_of(nm) < first]
    assert len(before) == 1 + 3 * first
    diff = [nm for nm in before if not np.array_equal(kept[nm], half[1][nm])]
    assert not diff, f"{local['schedule']}: the fp8 flag changed {diff}"
    assert not np.array_equal(kept[f"b{first}.out"], half[1][f"b{first}.out"])       # and the fp8 path really ran


def test_every_stage_from_the_first_fp8_block_within_twice_its_bound(local):
    from oracle import local_ref as lr
    A, kept, sched, want = local["A"], local["kept"], local["schedule"], local["want"]
    nb = len(A.blocks)
    have = set(kept) - {"patches"}
    expect = {"stem", "features"} | {f"b{i}.{t}" for i in range(nb) for t in ("dw", "gate", "out")}
    assert have == expect, f"{sched}: missing {sorted(expect - have)}, unexpected {sorted(have - expect)}"
    kinds = [st.kind for st, *_ in local["results"]]
    assert len(kinds) == 3 * len(want) + 1 and kinds.count("out_fp8") == len(want) and "out" not in kinds
    assert set(local["info"]) == {f"b{i}.out" for i in want}
    lines, failures = [], []
    for st, launch, got, ref, bound in local["results"]:
        assert got.shape == ref.shape == bound.shape and np.isfinite(got).all() and np.isfinite(bound).all(), st.name
        ratio, idx = lr.worst_ratio(got, ref, bound)
        line = f"{sched:18s} {st.name:12s} {st.kind:9s} {launch:40s} max|got-ref|/bound {ratio:6.3f} at {idx}"
        if st.kind == "out_fp8":
            fi = local["info"][st.name]
            line += f"; ambiguous {fi.ambiguous} of {fi.operands} ({fi.share:.1e})"
        lines.append(line)
        rep = lr.exceed_report(got, ref, bound, FACTOR)
        if rep:
            failures.append(f"stage {st.name} ({st.kind}), launch {launch}: {rep}")
    print("\n".join(lines))
    out_dir = os.environ.get("MMC_LOCAL_PARITY_OUT")      # tools: keep the table (profiles/local_parity.txt)
    if out_dir:
        with open(os.path.join(out_dir, f"local_parity_{sched}.txt"), "w") as f:
            f.write("\n".join(lines + failures) + "\n")
    assert not failures, f"{len(failures)} of {len(kinds)} stages exceed {FACTOR:g} x bound\n" + "\n".join(failures)


def test_ambiguous_share(local):
    """The bound's only allowance for an operand code that differs is not a hiding place: <= 1e-4 of a stage's operands."""
    from oracle import local_ref as lr
    assert lr.AMBIGUOUS_MAX == 1e-4
    for i in local["want"]:
        fi = local["info"][f"b{i}.out"]
        assert fi.operands == local["kept"][f"b{i}.dw"].size
        assert fi.share <= lr.AMBIGUOUS_MAX, f"{local['schedule']} b{i}.out: {fi.ambiguous} of {fi.operands} operands are ambiguous"
