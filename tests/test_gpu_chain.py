"""chain14_kernel: b7.projse .. b10.projse as ONE launch per lane.  Every phase of the chain is the body
of the launch it replaces, in the same order on the same arguments, so the features must equal those of separate launches
(MMC_CHAIN=0) bit for bit -- np.array_equal, no tolerance.  Shapes are the smallest at which the chain can go wrong: one workgroup,
a ragged lane split, a second (ragged) chunk."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_BATCH = 4
SIZES = (1, 3, 4, 5)          # 5 = two chunks of max_batch 4, the last one ragged
CHAIN_NAME = "b7.projse-b10.projse.chain|chain14"
MEMBERS = ["b7.projse"] + [f"b{i}.{half}" for i in (8, 9, 10) for half in ("mbconv", "projse")]


@contextmanager
def _env(**kv):
    """The schedule switches are read once, by the create call."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _create(sd, **kv):
    from mermaid_classifier_amd.backbone import Backbone
    env = {"MMC_CHAIN": None, "MMC_LANES": None, "MMC_KEEP_ACTIVATIONS": None}
    env.update(kv)
    with _env(**env):
        return Backbone(sd, device=0, max_batch=MAX_BATCH)


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(20261)
    return {k: rng.integers(0, 256, size=(5, 224, 224, 3), dtype=np.uint8) for k in "AB"}


@pytest.fixture(scope="module")
def handles(synth_sd):
    sd = {k: v.numpy() for k, v in synth_sd.items()}
    hs = {(lanes, chain): _create(sd, MMC_LANES=lanes, MMC_CHAIN=chain) for lanes in (None, "1") for chain in (None, "0")}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def unchained(handles, inputs):
    """Features of separate launches (MMC_CHAIN=0, default lanes), computed once: {(input, n): (n, 1280)}."""
    ref = handles[(None, "0")]
    return {(k, n): ref.extract(inputs[k][:n]).copy() for k in "AB" for n in SIZES}


def _names(bb, n):
    import torch
    p = torch.zeros((n, 224, 224, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 1280), dtype=torch.float32, device="cuda")
    return [name for name, _ in bb.profile(p, out)]


@pytest.mark.parametrize("lanes", [None, "1"], ids=["lanes-default", "lanes-1"])
@pytest.mark.parametrize("n", SIZES)
def test_chain_equals_separate_launches(handles, inputs, unchained, lanes, n):
    assert handles[(None, None)].lanes == 2 and handles[("1", None)].lanes == 1
    got = handles[(lanes, None)].extract(inputs["A"][:n])
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got, unchained[("A", n)])
    # (and the lane count does not move the separate launches either)
    assert np.array_equal(handles[(lanes, "0")].extract(inputs["A"][:n]), unchained[("A", n)])


def test_no_stale_data_between_calls(handles, inputs, unchained):
    """Input A, then B, then A through the SAME device buffers of one handle: a phase that read a stale cache line of the previous
    call, or another phase's leftover LDS, gives something else than the separate launches give for that input."""
    import torch
    bb = handles[(None, None)]
    buf = torch.empty((5, 224, 224, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((5, 1280), dtype=torch.float32, device="cuda")
    assert not np.array_equal(unchained[("A", 5)], unchained[("B", 5)])
    for k in "ABA":
        buf.copy_(torch.from_numpy(inputs[k]))
        out.zero_()
        bb.extract(buf, out=out)
        assert np.array_equal(out.cpu().numpy(), unchained[(k, 5)]), k


def test_graph_replay_of_the_chain(handles, inputs, unchained):
    """Five calls on the same buffers (the library captures a HIP graph on the third): the fifth equals the first."""
    import torch
    bb = handles[(None, None)]
    buf = torch.from_numpy(inputs["B"][:4]).cuda()
    out = torch.empty((4, 1280), dtype=torch.float32, device="cuda")
    before = bb.graph_stats()["captures"]
    runs = []
    for _ in range(5):
        out.zero_()
        bb.extract(buf, out=out)
        runs.append(out.cpu().numpy().copy())
    assert bb.graph_stats()["captures"] == before + 1
    assert np.array_equal(runs[4], runs[0])
    assert np.array_equal(runs[0], unchained[("B", 4)])


def test_launch_count(handles):
    """The chain is ONE profile entry in place of its seven members; MMC_CHAIN=0 launches the seven."""
    names = _names(handles[(None, None)], 1)
    assert [x for x in names if x.endswith(".chain|chain14")] == [CHAIN_NAME]
    assert not [x for x in names if x.split(".")[0] in ("b8", "b9", "b10")]
    assert "b7.projse" not in [x.split("|")[0] for x in names]
    sep = _names(handles[(None, "0")], 1)
    assert not [x for x in sep if "chain" in x]
    assert [x.split("|")[0] for x in sep if x.split("|")[0] in MEMBERS] == MEMBERS
    assert len(sep) == len(names) + 6
    # two lanes: one chain per lane
    assert [x for x in _names(handles[(None, None)], 4) if "chain" in x] == [CHAIN_NAME] * 2


def test_per_tensor_mode_keeps_separate_launches(synth_sd):
    """MMC_KEEP_ACTIVATIONS=1 hands every tensor out, so the chain is off there: test_gpu_layers.py's checks of the bodies'
    tensors run on the separate launches as before."""
    bb = _create({k: v.numpy() for k, v in synth_sd.items()}, MMC_KEEP_ACTIVATIONS="1")
    try:
        names = [x.split("|")[0] for x in _names(bb, 1)]
        assert not [x for x in names if "chain" in x]
        assert [x for x in names if x in MEMBERS] == MEMBERS
        assert np.abs(bb.read_activation("b9.dw", 196 * 672)).max() > 0
    finally:
        bb.close()
