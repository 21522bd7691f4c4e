"""CPU checks of ``oracle/local_ref.py`` (the stage references and per-element bounds ``tests/test_gpu_local.py`` holds the
kernels to), before any GPU run:

a. correct -- fed the fp32 oracle's own taps, every stage reproduces the oracle's next tap (<= 2e-5 relative per tensor, the
   figure ``test_fold_reproduces_oracle`` uses for fold against oracle); all stage kinds, both schedules' stage lists, B0 and B4;
b. sound   -- a float32 emulation that rounds to fp16 exactly where the error model says the kernels do (weights, values held
   between phases, stored outputs) and sums in another order stays within 1 x bound on every element of every stage;
c. sharp   -- seven deliberately wrong emulations (the bugs a per-tensor RMS gate lets through) each exceed 2 x bound."""

import numpy as np
import pytest
import torch

from oracle import efficientnet_b0_ref as ref
from oracle import local_ref as lr


def _weights(sd_t, arch):
    from mermaid_classifier_amd import weights
    A = weights.get_arch(arch)
    sd = {k: np.asarray(v.numpy(), np.float64) for k, v in sd_t.items() if k in weights.expected_shapes(A)}
    folded = weights.fold(sd, A)
    return lr.Weights(folded, A), folded, A


def _nhwc(name, t):
    a = t.numpy()
    if a.ndim == 4 and name.endswith(".gate"):
        return a.reshape(a.shape[0], a.shape[1])
    return a.transpose(0, 2, 3, 1) if a.ndim == 4 else a


# ---- a. correct -------------------------------------------------------------------------------------------------------

def _check_against_taps(W, arch, patches, taps, drop):
    kept = {k: _nhwc(k, v) for k, v in taps.items() if not drop(k)}
    kept["patches"] = patches
    stages = lr.plan(arch, [k for k in kept if k != "patches"])
    worst = {}
    for st in stages:
        got, bound = lr.run_stage(W, st, kept.__getitem__)
        want = _nhwc(st.name, taps[st.name]).astype(np.float64)
        assert got.shape == want.shape == bound.shape, st.name
        assert np.isfinite(bound).all() and (bound > 0).all(), st.name
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        worst[st.kind] = max(worst.get(st.kind, 0.0), rel)
        assert rel <= 2e-5, f"{st.name} ({st.kind}): {rel:.3g}"
    return stages, worst


def test_stages_reproduce_the_oracle_b0(synth_sd, oracle_net):
    W, _, _ = _weights(synth_sd, "b0")
    patches = ref.synthetic_patches(1, seed=42)
    taps = {}
    oracle_net.extract_features(ref.transformation(patches), taps=taps)
    unf, w1 = _check_against_taps(W, "b0", patches, taps, lambda k: False)
    fus, w2 = _check_against_taps(W, "b0", patches, taps, lambda k: k.endswith(".expand") or k in ("stem", "b0.out"))
    print("unfused", w1, "\nfused", w2)
    assert len(unf) == 65 and len(fus) == 48
    assert {s.kind for s in unf} | {s.kind for s in fus} == {"stem", "expand", "dw", "fused_dw", "stem_dw", "b1_fused", "gate",
                                                            "out", "features"}


def test_stages_reproduce_the_oracle_b4(synth_sd_b4):
    W, _, A = _weights(synth_sd_b4, "b4")
    patches = ref.natural_patches(1, seed=7)
    taps = {}
    ref.EfficientNetB0Ref(synth_sd_b4, arch="b4").extract_features(ref.transformation(patches), taps=taps)
    unf, _ = _check_against_taps(W, "b4", patches, taps, lambda k: False)
    fus, _ = _check_against_taps(W, "b4", patches, taps, lambda k: k.endswith(".expand"))
    assert len(fus) == 2 + 3 * 32 and len(unf) == len(fus) + 30
    assert [s.kind for s in fus if s.name in ("b0.dw", "b1.dw", "b2.dw")] == ["dw", "dw", "fused_dw"]


# ---- the emulation: float32, fp16 roundings where the model puts them, another summation order --------------------------------

def _q(x):
    return x.half().float()


class Emu:
    """What the device does according to the error model, stage by stage (NHWC float32).  ``mut`` names one deliberate bug."""

    def __init__(self, folded, A):
        self.t = {k: torch.from_numpy(v) for k, v in folded}
        self.A = A

    def w16(self, name):
        return _q(self.t[name])

    @staticmethod
    def linear(x, w, b, drop=None):
        acc = b.expand(*x.shape[:-1], w.shape[0]).clone()
        K = w.shape[1]
        for k0 in reversed(range(0, K, 32)):                      # k-steps of 32, last first
            part = x[..., k0:k0 + 32] @ w[:, k0:k0 + 32].T
            if drop is not None and k0 == drop[0]:
                part[..., drop[1]:drop[1] + 16] = 0               # mutant: this k-step is skipped for one 16-column tile
            acc = acc + part
        return acc

    @staticmethod
    def depthwise(x, w, b, s, swap_pad=False, drop_last_row_tap=None):
        k = w.shape[-1]
        Ho = -(-x.shape[1] // s)
        pb, pa = ref.same_pad(x.shape[1], k, s)
        if swap_pad:
            pb, pa = pa, pb
        xp = torch.nn.functional.pad(x, (0, 0, pb, pa, pb, pa))
        acc = b.expand(x.shape[0], Ho, Ho, x.shape[3]).clone()
        for ky in reversed(range(k)):
            for kx in reversed(range(k)):
                term = xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Ho - 1) * s + 1:s, :] * w[:, ky, kx]
                if drop_last_row_tap == (ky, kx):
                    term[:, -1] = 0
                acc = acc + term
        return acc

    @staticmethod
    def silu(x):
        return x * torch.sigmoid(x)

    def stem32(self, patches):
        x = torch.from_numpy(patches.astype(np.float32) - 128.0)
        xp = _q(self.t["stem.padval"]).view(1, 1, 1, 3).expand(x.shape[0], 225, 225, 3).clone()
        xp[:, :224, :224] = x
        w = self.w16("stem.weight").view(-1, 3, 3, 3)
        acc = self.t["stem.bias"].expand(x.shape[0], 112, 112, w.shape[0]).clone()
        for ky in reversed(range(3)):
            for kx in reversed(range(3)):
                acc = acc + xp[:, ky:ky + 223:2, kx:kx + 223:2, :] @ w[:, ky, kx, :].T
        return self.silu(acc)

    def stem(self, patches):
        return _q(self.stem32(patches))

    def expand(self, i, x):
        return _q(self.silu(self.linear(x, self.w16(f"b{i}.expand.weight"), self.t[f"b{i}.expand.bias"])))

    def dw(self, i, x, **mut):
        """-> (fp16 tensor, pool SUMS of the fp32 values before rounding)."""
        y = self.silu(self.depthwise(x, self.w16(f"b{i}.dw.weight"), self.t[f"b{i}.dw.bias"], self.A.blocks[i][1], **mut))
        return _q(y), y.sum(dim=(1, 2))

    def fused_dw(self, i, x, swap_channels=None, **mut):
        e = self.expand(i, x)
        if swap_channels is not None:
            c = swap_channels
            e[..., [c, c + 1]] = e[..., [c + 1, c]]
        return self.dw(i, e, **mut)

    def stem_dw(self, patches):
        return self.dw(0, self.stem(patches))

    def project32(self, i, d, g, skip=None, drop=None):
        y = self.linear(_q(d * g[:, None, None, :]), self.w16(f"b{i}.project.weight"), self.t[f"b{i}.project.bias"], drop)
        return y if skip is None else y + skip

    def b1_fused(self, d0, g0):
        return self.fused_dw(1, _q(self.project32(0, d0, g0)))

    def gate(self, i, pool_sum, hw):
        p = pool_sum * np.float32(1.0 / hw)
        r = self.silu(self.linear(p, self.w16(f"b{i}.se.reduce.weight"), self.t[f"b{i}.se.reduce.bias"]))
        return torch.sigmoid(self.linear(r, self.w16(f"b{i}.se.expand.weight"), self.t[f"b{i}.se.expand.bias"]))

    def out(self, i, d, g, skip=None, drop=None):
        return _q(self.project32(i, d, g, skip, drop))

    def features(self, x):
        y = self.silu(self.linear(x, self.w16("head.weight"), self.t["head.bias"]))
        return y.sum(dim=(1, 2)) * np.float32(1.0 / (x.shape[1] * x.shape[2]))

    def chain(self, patches, fused):
        """Every tensor the schedule keeps, and the fp32 pool sums the gate stages consumed."""
        kept, pools = {}, {}
        x = None
        if not fused:
            kept["stem"] = x = self.stem(patches)
        for i, (k, s, e, cin, cout) in enumerate(self.A.blocks):
            inp = x
            if fused and i == 0:
                d, ps = self.stem_dw(patches)
            elif fused and i == 1:
                d, ps = self.b1_fused(kept["b0.dw"], kept["b0.gate"])
            elif fused and e != 1:
                d, ps = self.fused_dw(i, x)
            else:
                if e != 1:
                    kept[f"b{i}.expand"] = x = self.expand(i, x)
                d, ps = self.dw(i, x)
            kept[f"b{i}.dw"], pools[i] = d, ps
            kept[f"b{i}.gate"] = g = self.gate(i, ps, d.shape[1] * d.shape[2])
            if not (fused and i == 0):
                kept[f"b{i}.out"] = x = self.out(i, d, g, inp if s == 1 and cin == cout else None)
        kept["features"] = self.features(x)
        return {k: v.numpy() for k, v in kept.items()}, pools


@pytest.fixture(scope="module")
def emu_b0(synth_sd):
    W, folded, A = _weights(synth_sd, "b0")
    emu = Emu(folded, A)
    patches = lr.parity_patches()
    with torch.no_grad():
        unf, pools = emu.chain(patches, fused=False)
        fus, _ = emu.chain(patches, fused=True)
    unf["patches"] = fus["patches"] = patches
    return W, emu, unf, fus, pools


# ---- b. sound -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["unfused", "fused"])
def test_honest_emulation_stays_within_one_bound(emu_b0, schedule):
    W, emu, unf, fus, _ = emu_b0
    kept = unf if schedule == "unfused" else fus
    stages = lr.plan("b0", [k for k in kept if k != "patches"])
    assert len(stages) == (65 if schedule == "unfused" else 48)
    lines, bad = [], []
    for st in stages:
        r, bound = lr.run_stage(W, st, kept.__getitem__)
        ratio, idx = lr.worst_ratio(kept[st.name], r, bound)
        lines.append(f"{st.name:12s} {st.kind:9s} {ratio:.3f}")
        if ratio > 1.0:
            bad.append(f"{st.name} ({st.kind}): {lr.exceed_report(kept[st.name], r, bound, 1.0)}")
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


# ---- c. sharp -----------------------------------------------------------------------------------------------------------

def _t32(a):
    return torch.from_numpy(np.asarray(a))


def _mutants(emu, kept, pools):
    """name -> (stage kind, block, mutated tensor); inputs are the honest chain's (unfused schedule: every tensor exists)."""
    k = {n: _t32(v) for n, v in kept.items() if n != "patches"}
    A = emu.A
    # block 1: 3x3 stride 2 (112 -> 56, pad (0, 1)); block 3: 5x5 stride 2 (56 -> 28); block 2 / 4: skip; block 5: 240 -> 80
    assert A.blocks[1][:2] == (3, 2) and A.blocks[3][:2] == (5, 2) and A.blocks[2][1] == 1 and A.blocks[5][3:] == (40, 80)
    g3_swapped = k["b3.gate"].clone()
    g3_swapped[1] = g3_swapped[0]
    skip_but_last = k["b1.out"].clone()
    skip_but_last[-1] = 0
    hw_in = kept["b3.expand"].shape[1] * kept["b3.expand"].shape[2]
    return {
        "depthwise padded on the wrong side (stride 2)": ("fused_dw", 1, emu.fused_dw(1, k["b0.out"], swap_pad=True)[0]),
        "one depthwise tap zeroed on the last output row": ("dw", 2, emu.dw(2, k["b2.expand"], drop_last_row_tap=(1, 2))[0]),
        "two adjacent expanded channels swapped": ("fused_dw", 3, emu.fused_dw(3, k["b2.out"], swap_channels=6)[0]),
        "one 32-wide k-step of a project dropped for one 16-column tile": ("out", 5, emu.out(5, k["b5.dw"], k["b5.gate"], drop=(64, 16))),
        "skip omitted for the last patch": ("out", 2, emu.out(2, k["b2.dw"], k["b2.gate"], skip_but_last)),
        "patch 0's gate used for patch 1": ("out", 3, emu.out(3, k["b3.dw"], g3_swapped)),
        "pool divided by HW_in instead of HW_out (stride 2)": ("gate", 3, emu.gate(3, pools[3], hw_in)),
    }


def test_wrong_kernels_exceed_twice_the_bound(emu_b0):
    W, emu, unf, _, pools = emu_b0
    with torch.no_grad():
        muts = _mutants(emu, unf, pools)
    assert len(muts) == 7
    refs = {
        ("fused_dw", 1): lambda: lr.fused_dw(W, 1, unf["b0.out"]),
        ("dw", 2): lambda: lr.dw(W, 2, unf["b2.expand"]),
        ("fused_dw", 3): lambda: lr.fused_dw(W, 3, unf["b2.out"]),
        ("out", 5): lambda: lr.out(W, 5, unf["b5.dw"], unf["b5.gate"]),
        ("out", 2): lambda: lr.out(W, 2, unf["b2.dw"], unf["b2.gate"], unf["b1.out"]),
        ("out", 3): lambda: lr.out(W, 3, unf["b3.dw"], unf["b3.gate"]),
        ("gate", 3): lambda: lr.gate(W, 3, unf["b3.dw"]),
    }
    escaped = []
    for name, (kind, blk, got) in muts.items():
        r, bound = refs[(kind, blk)]()
        got = got.numpy()
        ratio, idx = lr.worst_ratio(got, r, bound)
        n_over = int((np.abs(got - r) > 2 * bound).sum())
        print(f"{name:64s} b{blk}.{kind:9s} max ratio {ratio:10.1f}, {n_over} elements over 2 x bound")
        if n_over == 0:
            escaped.append(name)
    assert not escaped, f"the bound is too loose to catch: {escaped}"


def test_mutants_hit_where_the_bug_is(emu_b0):
    """The excess of the last-row mutant sits on the last output row only, the dropped k-step's on its 16 columns only: what
    the failure message's row / channel breakdown localises."""
    W, emu, unf, _, _ = emu_b0
    with torch.no_grad():
        got = emu.dw(2, _t32(unf["b2.expand"]), drop_last_row_tap=(1, 2))[0].numpy()
        got5 = emu.out(5, _t32(unf["b5.dw"]), _t32(unf["b5.gate"]), drop=(64, 16)).numpy()
    r, bound = lr.dw(W, 2, unf["b2.expand"])
    over = np.abs(got - r) > 2 * bound
    assert over[:, -1].any() and not over[:, :-1].any()
    assert "by row: 55:" in lr.exceed_report(got, r, bound)
    r, bound = lr.out(W, 5, unf["b5.dw"], unf["b5.gate"])
    over = np.abs(got5 - r) > 2 * bound
    assert over[..., 16:32].any() and not over[..., :16].any() and not over[..., 32:].any()
