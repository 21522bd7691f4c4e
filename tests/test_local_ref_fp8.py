"""CPU checks of the ``out_fp8`` stage of ``oracle/local_ref.py`` (rule 7: the reference and per-element bound
``tests/test_gpu_local_fp8.py`` holds ``pw_gemm_fp8_kernel`` to), before any GPU run:

a. codec   -- the numpy e4m3 encoder against ``mmc_fp8_e4m3_encode`` on every decoded code, every midpoint between adjacent
   codes +- 1 fp32 ulp, and a random sweep; the decoder against torch's ``float8_e4m3fn``;
b. sound   -- a float32 emulation of the kernel (the same operand codes, k-steps of 128 summed last step first, the epilogue in
   fp32, an fp16 store) stays within 1 x bound on every element of every fp8 block, with ``MMC_FP8_MAXH`` unset (blocks 22-31)
   and set to 14 (blocks 10-31); at most 1e-4 of a stage's operands are ambiguous; an all-zero pixel row gives bias (+ skip);
c. sharp   -- ten deliberately wrong emulations each exceed 2 x bound, and where the bug has a place the excess sits there.

Inputs: the float64 oracle's B4 taps on ``lr.parity_patches()``, rounded the way the device holds them (fp16 depthwise tensor in
the scaled domain, read out through the library's fp32 1 / log2(e); fp32 gate; fp16 skip)."""

import numpy as np
import pytest
import torch

from oracle import efficientnet_b0_ref as ref
from oracle import local_ref as lr

F32 = np.float32
FP8_BLOCKS = {"maxh7": range(22, 32), "maxh14": range(10, 32)}


# ---- a. codec -----------------------------------------------------------------------------------------------------------

def _lib_encode(x):
    from mermaid_classifier_amd import _lib
    x = np.ascontiguousarray(x, dtype=F32)
    out = np.zeros(len(x), np.uint8)
    _lib.check(_lib.lib().mmc_fp8_e4m3_encode(x.ctypes.data, out.ctypes.data, len(x)))
    return out


def test_decoder_matches_torch_float8():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    got = lr.e4m3_decode(codes)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and int(np.isnan(got).sum()) == 2
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
    assert got[0x7E] == 448 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6


def test_encoder_matches_the_library_bit_for_bit():
    codes = np.arange(256, dtype=np.uint8)
    vals = lr.e4m3_decode(codes)
    finite = ~np.isnan(vals)
    # every decoded code encodes to itself, in both implementations (NaN -> 0x7F)
    assert np.array_equal(lr.e4m3_encode(vals[finite]), codes[finite])
    assert np.array_equal(lr.e4m3_encode(vals), _lib_encode(vals))
    # every midpoint between adjacent codes, and one fp32 ulp to either side; both signs; the saturation edge
    pos = lr.e4m3_decode(np.arange(127, dtype=np.uint8)).astype(np.float64)
    mids = (0.5 * (pos[:-1] + pos[1:])).astype(F32)
    assert np.array_equal(mids.astype(np.float64), 0.5 * (pos[:-1] + pos[1:]))       # exact in fp32
    edge = np.array([448, 464, 480, 1e9, np.inf, 2.0 ** -10, 2.0 ** -11, 0.0], F32)
    pts = np.concatenate([mids, np.nextafter(mids, F32(np.inf)), np.nextafter(mids, F32(0)), edge,
                          np.nextafter(edge[:4], F32(np.inf)), np.nextafter(edge[:4], F32(0))])
    pts = np.concatenate([pts, -pts])
    got, want = lr.e4m3_encode(pts), _lib_encode(pts)
    assert np.array_equal(got, want), pts[got != want][:8]
    k = np.arange(126)
    tie = lr.e4m3_encode(mids)
    assert np.array_equal(tie, np.where(k % 2 == 0, k, k + 1))                       # a tie goes to the even code
    assert np.array_equal(lr.e4m3_encode(np.nextafter(mids, F32(np.inf))), k + 1)
    assert np.array_equal(lr.e4m3_encode(np.nextafter(mids, F32(0))), k)
    # a random sweep: scales from subnormal to saturating, and raw bit patterns (NaN, infinities, fp32 subnormals)
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(0, s, 50000) for s in (1e-3, 1e-2, 1, 30, 300)]).astype(F32)
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(F32)
    for sweep in (x, bits):
        got, want = lr.e4m3_encode(sweep), _lib_encode(sweep)
        assert np.array_equal(got, want), sweep[got != want][:8]


# ---- the inputs: what the device would hold --------------------------------------------------------------------------------

def _nhwc(t):
    return t.numpy().transpose(0, 2, 3, 1)


@pytest.fixture(scope="module")
def b4(synth_sd_b4):
    """W, folded fp32 tensors by name, and per fp8 block: (read-out of the fp16 depthwise tensor, fp32 gate, fp16 skip or None)."""
    from mermaid_classifier_amd import weights
    A = weights.get_arch("b4")
    sd = {k: np.asarray(v.numpy(), np.float64) for k, v in synth_sd_b4.items() if k in weights.expected_shapes(A)}
    folded = weights.fold(sd, A)
    W = lr.Weights(folded, A)
    taps = {}
    with torch.no_grad():
        ref.EfficientNetB0Ref(synth_sd_b4, arch="b4").extract_features(ref.transformation(lr.parity_patches()), taps=taps)
    ins = {}
    for i in FP8_BLOCKS["maxh14"]:
        k, s, e, cin, cout = A.blocks[i]
        d16 = (_nhwc(taps[f"b{i}.dw"]).astype(np.float64) * lr.LOG2E).astype(np.float16)
        read = d16.astype(F32) * F32(1.0 / lr.LOG2E)
        g = taps[f"b{i}.gate"].numpy().reshape(3, cin * e).astype(F32)
        skip = _nhwc(taps[f"b{i - 1}.out"]).astype(np.float16).astype(F32) if s == 1 and cin == cout else None
        ins[i] = (read, g, skip)
    return W, dict(folded), A, ins


# ---- the emulation: float32, the kernel's order of operations -----------------------------------------------------------------

_POS = lr.e4m3_decode(np.arange(127, dtype=np.uint8))


def _encode_toward_zero(t):
    idx = np.clip(np.searchsorted(_POS, np.abs(t), side="right") - 1, 0, 126).astype(np.uint8)
    return idx | np.where(np.signbit(t), 0x80, 0).astype(np.uint8)


def emulate(folded, i, read, g, skip, mut=None, arg=None):
    """pw_gemm_fp8_kernel on (b{i}.dw, b{i}.gate, skip) in float32 -> fp16 output as float32, NHWC.  ``mut`` names one bug."""
    w, b = folded[f"b{i}.project.weight"].astype(F32), folded[f"b{i}.project.bias"].astype(F32)
    N, K = w.shape
    n, h, _, _ = read.shape
    hw, M = h * h, n * h * h
    # weights
    if mut == "weight scale amax / 447":
        sc = (np.abs(w).max(axis=1) / F32(447.0)).astype(F32)
        cw, sw = lr.e4m3_encode(w / sc[:, None]), (sc.astype(np.float64) / lr.LOG2E).astype(F32)
    else:
        cw, sw = lr.fp8_weight_codes(w)
    if mut == "sw without 1 / log2(e)":
        sw = (sw.astype(np.float64) * lr.LOG2E).astype(F32)
    qw = lr.e4m3_decode(cw)
    if mut == "last fragment of N = 272 from fragment 15":
        assert N == 272
        qw = qw.copy()
        qw[256:272] = qw[240:256]
    # activations
    d16 = (read * F32(lr.LOG2E)).astype(np.float16).reshape(M, K)
    patch = np.arange(M) // hw
    if mut == "patch 0's gate in the fragment that straddles patches 0 and 1":
        assert hw == 49
        patch[49:64] = 0
    v = d16.astype(F32) * g[patch]
    kfull = K // 128 * 128
    mx = np.abs(v[:, :kfull] if mut == "row maximum over the full k-steps only" else v).max(axis=1)
    pos = mx > 0
    inv = np.where(pos, F32(447.0) / np.where(pos, mx, F32(1)), F32(0)).astype(F32)
    sx = np.where(pos, mx * (F32(1.0) / F32(447.0)), F32(0)).astype(F32)
    t = v * inv[:, None]
    qx = lr.e4m3_decode(_encode_toward_zero(t) if mut == "activations truncated toward zero" else lr.e4m3_encode(t))
    # k-steps of 128, the last one first
    acc = np.zeros((M, N), F32)
    for k0 in reversed(range(0, K, 128)):
        part = qx[:, k0:k0 + 128] @ qw[:, k0:k0 + 128].T
        if mut == "partial last k-step dropped for one fragment" and k0 == kfull:
            part[:, 16 * arg:16 * arg + 16] = 0
        acc = acc + part
    if mut == "the neighbouring row's sx":
        sx = sx[np.minimum(np.arange(M) ^ 1, M - 1)]
    y = acc * sx[:, None] * sw[None, :] + b[None, :]
    if skip is not None:
        s = skip.reshape(M, N).copy()
        if mut == "skip omitted for the last patch":
            s[patch == n - 1] = 0
        y = y + s
    assert y.dtype == F32
    return y.astype(np.float16).astype(F32).reshape(n, h, h, N)


# ---- b. sound -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", list(FP8_BLOCKS))
def test_honest_emulation_stays_within_one_bound(b4, schedule):
    W, folded, A, ins = b4
    shapes, lines, bad = set(), [], []
    for i in FP8_BLOCKS[schedule]:
        read, g, skip = ins[i]
        got = emulate(folded, i, read, g, skip)
        r, bound, info = lr.out_fp8(W, i, read, g, skip)
        assert got.shape == r.shape == bound.shape and np.isfinite(bound).all() and (bound > 0).all()
        ratio, idx = lr.worst_ratio(got, r, bound)
        lines.append(f"b{i}.out K {read.shape[-1]:4d} N {got.shape[-1]:3d} HW {read.shape[1] ** 2:3d} skip {int(skip is not None)} "
                     f"max|got-ref|/bound {ratio:.3f}; ambiguous {info.ambiguous} of {info.operands} ({info.share:.2e})")
        shapes.add((read.shape[-1], got.shape[-1], read.shape[1] ** 2, skip is not None))
        if ratio > 1.0:
            bad.append(f"b{i}.out: {lr.exceed_report(got, r, bound, 1.0)}")
        assert info.operands == read.size and info.share <= lr.AMBIGUOUS_MAX, lines[-1]
    print("\n".join(lines))
    assert not bad, "\n".join(bad)
    want = {(960, 272, 49, False), (1632, 272, 49, True), (1632, 448, 49, False), (2688, 448, 49, True)}
    if schedule == "maxh14":
        want |= {(336, 112, 196, False), (672, 112, 196, True), (672, 160, 196, False), (960, 160, 196, True)}
    assert shapes == want


def test_plan_emits_out_fp8_for_the_fp8_blocks(b4):
    W, folded, A, ins = b4
    have = ["stem", "features"] + [f"b{i}.{t}" for i in range(len(A.blocks)) for t in ("dw", "gate", "out")]
    stages = lr.plan("b4", have, fp8_blocks=set(FP8_BLOCKS["maxh7"]))
    assert [s.block for s in stages if s.kind == "out_fp8"] == list(range(22, 32))
    assert [s.block for s in stages if s.kind == "out"] == list(range(22))
    assert [(s.kind, s.block) for s in lr.plan("b4", have)] == [("out" if s.kind == "out_fp8" else s.kind, s.block) for s in stages]
    st = next(s for s in stages if s.name == "b23.out")
    assert st.inputs == ("b23.dw", "b23.gate", "b22.out")
    read, g, skip = ins[23]
    info = {}
    r, bound = lr.run_stage(W, st, {"b23.dw": read, "b23.gate": g, "b22.out": skip}.__getitem__, info)
    r2, bound2, fi = lr.out_fp8(W, 23, read, g, skip)
    assert np.array_equal(r, r2) and np.array_equal(bound, bound2) and info == {"b23.out": fi}


def test_recovery_of_the_fp16_bits_is_asserted(b4):
    W, folded, A, ins = b4
    read, g, skip = ins[22]
    bad = read.copy()
    bad[0, 0, 0, 0] = np.nextafter(bad[0, 0, 0, 0], F32(np.inf))           # one fp32 ulp off an fp16 value times the library's factor
    with pytest.raises(ValueError, match="cannot be recovered"):
        lr.out_fp8(W, 22, bad, g, skip)


def test_all_zero_pixel_row(b4):
    """mx == 0 (codes 0, sx = 0; the output is bias + skip): the backbone's inputs cannot produce such a row, so only the
    emulation covers it."""
    W, folded, A, ins = b4
    read, g, skip = ins[23]
    read = read.copy()
    read[1, 3, 4, :] = 0
    read[2, 6, 6, :] = -0.0
    got = emulate(folded, 23, read, g, skip)
    r, bound, info = lr.out_fp8(W, 23, read, g, skip)
    assert np.isfinite(r).all() and np.isfinite(got).all()
    assert np.array_equal(r[1, 3, 4], folded["b23.project.bias"].astype(np.float64) + skip[1, 3, 4])
    assert lr.worst_ratio(got, r, bound)[0] <= 1.0


# ---- c. sharp -------------------------------------------------------------------------------------------------------------

# name -> (block, argument)
MUTANTS = {
    "partial last k-step dropped for one fragment, K = 960 (k >= 896)": ("partial last k-step dropped for one fragment", 22, 1),
    "partial last k-step dropped for one fragment, K = 336 (k >= 256)": ("partial last k-step dropped for one fragment", 10, 6),
    "row maximum over the full k-steps only": ("row maximum over the full k-steps only", 22, None),
    "the neighbouring row's sx": ("the neighbouring row's sx", 23, None),
    "patch 0's gate in the fragment that straddles patches 0 and 1": ("patch 0's gate in the fragment that straddles patches 0 and 1", 23, None),
    "last fragment of N = 272 from fragment 15": ("last fragment of N = 272 from fragment 15", 23, None),
    "skip omitted for the last patch": ("skip omitted for the last patch", 24, None),
    "activations truncated toward zero": ("activations truncated toward zero", 31, None),
    "sw without 1 / log2(e)": ("sw without 1 / log2(e)", 30, None),
    "weight scale amax / 447": ("weight scale amax / 447", 25, None),
}


@pytest.fixture(scope="module")
def mutants(b4):
    W, folded, A, ins = b4
    res = {}
    for name, (mut, i, arg) in MUTANTS.items():
        read, g, skip = ins[i]
        got = emulate(folded, i, read, g, skip, mut, arg)
        r, bound, _ = lr.out_fp8(W, i, read, g, skip)
        res[name] = (i, got, r, bound, np.abs(got - r) > 2 * bound)
    return res


def test_wrong_kernels_exceed_twice_the_bound(mutants):
    assert len(mutants) == 10
    escaped = []
    for name, (i, got, r, bound, over) in mutants.items():
        ratio, idx = lr.worst_ratio(got, r, bound)
        print(f"{name:66s} b{i}.out max ratio {ratio:10.1f}, {int(over.sum())} of {over.size} elements over 2 x bound")
        if not over.any():
            escaped.append(name)
    assert not escaped, f"the bound is too loose to catch: {escaped}"


def test_mutants_hit_where_the_bug_is(mutants):
    """What the failure message's row / column / channel breakdown localises."""
    for name, frag, K in (("partial last k-step dropped for one fragment, K = 960 (k >= 896)", 1, 960),
                          ("partial last k-step dropped for one fragment, K = 336 (k >= 256)", 6, 336)):
        i, got, r, bound, over = mutants[name]
        assert i in (10, 22) and K == {10: 336, 22: 960}[i]
        cols = np.zeros(over.shape[-1], bool)
        cols[16 * frag:16 * frag + 16] = True
        assert over[..., cols].any() and not over[..., ~cols].any(), name
    i, got, r, bound, over = mutants["patch 0's gate in the fragment that straddles patches 0 and 1"]
    rows = over.reshape(-1, over.shape[-1]).any(axis=1)                    # 147 GEMM rows: patch 1 starts at row 49
    assert rows[49:64].any() and not rows[:49].any() and not rows[64:].any()
    assert "by patch: 1:" in lr.exceed_report(got, r, bound)
    i, got, r, bound, over = mutants["last fragment of N = 272 from fragment 15"]
    assert over[..., 256:].any() and not over[..., :256].any()
    i, got, r, bound, over = mutants["skip omitted for the last patch"]
    assert over[2].any() and not over[:2].any()
