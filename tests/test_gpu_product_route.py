"""-m gpu: the product pass equals per-tensor mode bit for bit.

``tests/test_gpu_local.py`` checks every launch of per-tensor mode (MMC_KEEP_ACTIVATIONS=1) element by element.  The product pass runs
the same bodies otherwise: blocks 11-15 and the head as ONE ``tail7`` launch with the tensors resident in LDS, blocks 7-10 as one
chain per lane, two lanes, a HIP graph.  Every phase of those launches is the body of the per-tensor launch, the values handed from
block to block are the same fp16 numbers whether they stay in LDS or go through HBM, and the debug pointers only add stores -- so the
features must be equal, ``np.array_equal``, no tolerance.  One wrong border pixel in one 7x7 map sits far below the end-to-end
gates of ``tests/test_gpu_parity.py``; it does not sit below this.

Shapes: max_batch 4 and 1, 3, 4, 5 patches -- one workgroup, a ragged 2 + 1 lane split, full lanes, a second (ragged) chunk."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_BATCH = 4
SIZES = (1, 3, 4, 5)
SPLIT = {"MMC_TAIL_B11": "0", "MMC_B1_PLANAR": "0"}
SWITCHES = ("MMC_KEEP_ACTIVATIONS", "MMC_TAIL_B11", "MMC_B1_PLANAR", "MMC_CHAIN", "MMC_LANES", "MMC_GRAPH", "MMC_TAIL", "MMC_TAIL_FULL")
CHAIN = "b7.projse-b10.projse.chain|chain14"


@contextmanager
def _env(**kv):
    """The schedule switches are read once, by the create call; everything not named is cleared for it."""
    want = {k: None for k in SWITCHES}
    want.update(kv)
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
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
    with _env(**kv):
        return Backbone(sd, device=0, max_batch=MAX_BATCH)


def _entries(bb, n):
    import torch
    p = torch.zeros((n, 224, 224, 3), dtype=torch.uint8, device="cuda")
    return [name for name, _ in bb.profile(p, torch.empty((n, bb.feature_dim), dtype=torch.float32, device="cuda"))]


@pytest.fixture(scope="module")
def patches():
    """The three parity patches (image-like, white noise, border-heavy) and two seeded uint8 noise patches."""
    from oracle import local_ref as lr
    noise = np.random.default_rng(20262).integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8)
    return np.concatenate([lr.parity_patches(), noise])


@pytest.fixture(scope="module")
def b0(synth_sd):
    """{(schedule, mode): handle} on the same weights: the default schedule and MMC_TAIL_B11=0 + MMC_B1_PLANAR=0, product and per-tensor."""
    sd = {k: v.numpy() for k, v in synth_sd.items()}
    hs = {("default", "product"): _create(sd), ("default", "per-tensor"): _create(sd, MMC_KEEP_ACTIVATIONS="1"),
          ("split", "product"): _create(sd, **SPLIT), ("split", "per-tensor"): _create(sd, MMC_KEEP_ACTIVATIONS="1", **SPLIT)}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def per_tensor(b0, patches):
    """Per-tensor mode's features, computed once: {(schedule, n): (n, 1280)}."""
    return {(s, n): b0[(s, "per-tensor")].extract(patches[:n]).copy() for s in ("default", "split") for n in SIZES}


def test_the_handles_run_the_routes_they_are_named_for(b0):
    """Otherwise the equalities below could pass on a schedule that quietly fell back."""
    prod = b0[("default", "product")]
    assert prod.lanes == 2
    for n, lanes in ((1, 1), (4, 2)):
        names = _entries(prod, n)
        assert [x for x in names if ".tail" in x] == ["b11all-head.tail|tail7"] * lanes, names
        assert [x for x in names if "chain" in x] == [CHAIN] * lanes, names
        assert names.count("b0.project+b1.mbconv|mb1") == lanes and names.count("b1.project|thin_proj") == lanes
        assert not [x for x in names if x.split(".")[0] in ("b8", "b9", "b10", "b11", "b12", "b13", "b14", "b15", "head")]
    keep = b0[("default", "per-tensor")]
    assert keep.lanes == 1
    names = _entries(keep, 4)
    assert [x for x in names if ".tail" in x] == ["b11.tail|tail7"] + [f"b{i}.tail|tail7" for i in (12, 13, 14, 15)] + ["head.tail|tail7"]
    assert not [x for x in names if "chain" in x or x.startswith("b11.mbconv")]
    assert "b0.project+b1.mbconv|mb1<planar>" in names and "b1.project|thin_proj<planar>" in names
    names = _entries(b0[("split", "product")], 4)
    assert [x for x in names if ".tail" in x] == ["b11-head.tail|tail7"] * 2, names
    assert len([x for x in names if x.startswith("b11.mbconv|mbconv_a<5,2,")]) == 2 and [x for x in names if "chain" in x] == [CHAIN] * 2
    names = _entries(b0[("split", "per-tensor")], 4)
    assert [x for x in names if x.startswith("b11.")] == [[x for x in names if x.startswith("b11.mbconv|mbconv_a<5,2,")][0], "b11.tail|tail7"]
    assert "b0.project+b1.mbconv|mb1" in names and "b1.project|thin_proj" in names


@pytest.mark.parametrize("schedule", ["default", "split"])
@pytest.mark.parametrize("n", SIZES)
def test_product_pass_equals_per_tensor_mode(b0, patches, per_tensor, schedule, n):
    got = b0[(schedule, "product")].extract(patches[:n])
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    diff = np.nonzero(got != per_tensor[(schedule, n)])
    print(f"{schedule} n {n}: {len(diff[0])} of {got.size} features differ"
          + (f", patches {sorted(set(diff[0].tolist()))}, max |d| {np.abs(got - per_tensor[(schedule, n)]).max():.3g}" if len(diff[0]) else ""))
    assert np.array_equal(got, per_tensor[(schedule, n)])


@pytest.mark.parametrize("schedule", ["default", "split"])
def test_graph_replay_equals_per_tensor_mode(b0, patches, per_tensor, schedule):
    """Five calls on the same device buffers (the library captures a HIP graph on the third): the fifth equals the first, and both
    equal per-tensor mode."""
    import torch
    bb = b0[(schedule, "product")]
    buf = torch.from_numpy(patches[:4]).cuda()
    out = torch.empty((4, bb.feature_dim), dtype=torch.float32, device="cuda")
    before = bb.graph_stats()["captures"]
    runs = []
    for _ in range(5):
        out.zero_()
        bb.extract(buf, out=out)
        runs.append(out.cpu().numpy().copy())
    assert bb.graph_stats()["captures"] == before + 1
    assert np.array_equal(runs[4], runs[0])
    assert np.array_equal(runs[0], per_tensor[(schedule, 4)])


def test_b4_product_pass_equals_per_tensor_mode(synth_sd_b4):
    """B4 has no tail7 and no chain: lanes and the graph are all that separates the two."""
    from oracle import local_ref as lr
    sd = {k: v.numpy() for k, v in synth_sd_b4.items()}
    three = lr.parity_patches()
    prod, keep = _create(sd), _create(sd, MMC_KEEP_ACTIVATIONS="1")
    try:
        assert prod.arch == keep.arch == "b4" and prod.lanes == 2 and keep.lanes == 1
        got = prod.extract(three)
        assert np.isfinite(got).all() and np.abs(got).max() > 0
        assert np.array_equal(got, keep.extract(three))
    finally:
        prod.close()
        keep.close()
