#!/usr/bin/env python3
"""GPU box: one sha256 line per backbone schedule over the features it computes, with the handle's workspace bytes and its launch
list, to compare two builds of the library bit for bit (MMC_LIBRARY names the build; run it once per build in one visit; the two
outputs must be identical line for line: profiles/backbone_pack_bits.txt).

Synthetic weights (synthetic.py + the committed BN statistics); B0 handles with max_batch 8, B4 handles with max_batch 4.  Every
case is a fresh handle with its switches set before create: one extract of 5 patches (3 natural + 2 noise; two lanes, 3 + 2), one
of 1 patch, one profile pass at 1 patch.  The per-tensor cases (MMC_KEEP_ACTIVATIONS=1) also hash every activation the schedule
keeps (not the *.clk cycle counters).  A minute or two in all."""
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from mermaid_classifier_amd import weights  # noqa: E402
from mermaid_classifier_amd.backbone import Backbone  # noqa: E402
from mermaid_classifier_amd.synthetic import synthetic_state_dict  # noqa: E402
from oracle import efficientnet_b0_ref as ref  # noqa: E402
from oracle import local_ref as lr  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
SD = {
    "b0": synthetic_state_dict(0, dict(np.load(GOLDEN / "synth_bn_stats.npz"))),
    "b4": synthetic_state_dict(0, {k: v.astype(np.float32) for k, v in np.load(GOLDEN / "synth_bn_stats_b4.npz").items()}, arch="b4"),
}
MAX_BATCH = {"b0": 8, "b4": 4}
PATCHES = np.concatenate([ref.natural_patches(3, seed=7), ref.synthetic_patches(2, seed=42)])
# the single knobs of tests/test_gpu_parity.py::test_every_schedule_variant_meets_the_same_gates
B0_KNOBS = ["MMC_FUSE_B0", "MMC_SE_SMALL", "MMC_PROJSE", "MMC_TAIL_B11", "MMC_TAIL_FULL", "MMC_TAIL", "MMC_MB_DOT2", "MMC_MID14", "MMC_MID14=2",
            "MMC_MID14M=1", "MMC_MID14M=0", "MMC_MBT4=0", "MMC_MB1", "MMC_MBT", "MMC_MBT2", "MMC_THIN_PROJ", "MMC_B1_PLANAR", "MMC_GRAPH", "MMC_LANES"]


def knob_env(knob):
    if "=" in knob:
        k, v = knob.split("=")
        return {k: v}
    return {knob: "1" if knob == "MMC_LANES" else "0"}


def digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def case(name, arch, env, precision="fp16", keep=False):
    env = dict(env, **({"MMC_KEEP_ACTIVATIONS": "1"} if keep else {}))
    os.environ.update(env)
    try:
        bb = Backbone(SD[arch], device=0, max_batch=MAX_BATCH[arch], precision=precision)
    finally:
        for k in env:
            os.environ.pop(k, None)
    try:
        f5 = bb.extract(PATCHES)
        print(f"{name}: workspace_bytes {bb.workspace_bytes} lanes {bb.lanes}")
        print(f"{name}: features n=5 {digest(f5)}")
        if keep:
            A = weights.get_arch(arch)
            found = []
            for nm in ["stem"] + [f"b{i}.{t}" for i in range(len(A.blocks)) for t in ("expand", "dw", "gate", "out")]:
                try:
                    act = bb.read_activation(nm, int(np.prod(lr.tensor_shape(arch, nm, len(PATCHES)))))
                except ValueError:
                    continue      # not kept by this schedule
                found.append(nm)
                print(f"{name}: activation {nm} [{act.size}] {digest(act)}")
            print(f"{name}: activations kept: {' '.join(found)}")
        print(f"{name}: features n=1 {digest(bb.extract(PATCHES[:1]))}")
        dev = torch.from_numpy(PATCHES[:1]).cuda()
        launches = bb.profile(dev, torch.empty((1, bb.feature_dim), dtype=torch.float32, device="cuda"))
        print(f"{name}: launches {' '.join(nm for nm, _ in launches)}")
    finally:
        bb.close()
    sys.stdout.flush()


case("b0 default", "b0", {})
for knob in B0_KNOBS:
    e = knob_env(knob)
    case("b0 " + " ".join(f"{k}={v}" for k, v in e.items()), "b0", e)
case("b0 MMC_FUSE=0", "b0", {"MMC_FUSE": "0"})
case("b0 MMC_CHAIN=0", "b0", {"MMC_CHAIN": "0"})
case("b4 default", "b4", {})
for k in ("MMC_FUSE", "MMC_THIN_PROJ", "MMC_PROJSE"):
    case(f"b4 {k}=0", "b4", {k: "0"})
case("b4 fp8", "b4", {}, precision="fp8")
# per-tensor mode on the schedules of tests/test_gpu_local.py
case("keep b0-fused", "b0", {}, keep=True)
case("keep b0-unfused", "b0", {"MMC_FUSE": "0"}, keep=True)
case("keep b0-fused-mfma-dw", "b0", {"MMC_MID14M": "1", "MMC_MBT4": "1"}, keep=True)
case("keep b4", "b4", {}, keep=True)
case("keep b4-unfused", "b4", {"MMC_FUSE": "0"}, keep=True)
