"""sgx_psd_* / sgx_csd_*: Welch-averaged spectra per bin (include/sgx.h), through the C ABI.

The contract is that the output is a pure function of the rows: the batch calls equal the host reference of the header's sum order
(tests/psd_reference.py: a float32 chain per block of 32 frames, a float64 chain over a column's blocks, one divide, one cast) over the
engine's own sgx_stft_batch / sgx_stft_batch_complex rows bit for bit -- on every transform family, for every group, sub-range,
compute-unit limit and stream, and across the seams of the workspace's ranges.  The values are held to the float64 mean of the same rows
within the header's 35 * 2^-24 bound, and end to end to the float64 truth within the rows' own allowance (tests/conftest.py) carried
through the products.  No context runs a fused mode in this build: sgx_psd_fused and sgx_csd_fused answer 0 everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import psd_reference as ref
from conftest import FLOOR_K16, FLOOR_WIDE, PEAK_FLOOR, REL_TOL
from psd_reference import BOUND, SIZE_MAX
from spectrogram_rs_amd import SpectrogramEngine, _lib
from test_gpu_complex import truth_complex

pytestmark = pytest.mark.gpu

SR = 48000.0
FRAMES = 80
WORKSPACE_BYTES = 192 << 20          # include/sgx.h: the bounded workspace

_W2048 = dict(window_samples=2048, hop_samples=256)
# name: (engine keyword arguments, frames, the rows' floor)
CASES = {
    "w2048_h256_mono": (dict(_W2048, channels=1), FRAMES, PEAK_FLOOR),
    "w2048_h256_lr": (dict(_W2048, channels=2), FRAMES, PEAK_FLOOR),
    "w2048_h200_lr": (dict(window_samples=2048, hop_samples=200, channels=2), FRAMES, FLOOR_WIDE),
    "w2048_ch4": (dict(_W2048, channels=4), FRAMES, FLOOR_WIDE),
    "w2048_ch8": (dict(_W2048, channels=8), FRAMES, FLOOR_WIDE),
    "w2048_h256_lr_unfused": (dict(_W2048, channels=2, fused_render=False), FRAMES, PEAK_FLOOR),
    "w2048_h256_lr_generic": (dict(_W2048, channels=2, force_generic=True), FRAMES, FLOOR_WIDE),
    "w2048_h256_mono_paired": (dict(_W2048, channels=1, paired_frames=True), FRAMES, FLOOR_WIDE),
    "w2048_h256_mono_complex": (dict(_W2048, channels=1, complex_mono=True), FRAMES, FLOOR_WIDE),
    "w2400_h93_lr": (dict(window_samples=2400, hop_samples=93, channels=2), FRAMES, FLOOR_WIDE),
    "w1024_h256_lr": (dict(window_samples=1024, hop_samples=256, channels=2), FRAMES, FLOOR_WIDE),
    "w1102_chirpz": (dict(window_samples=1102, hop_samples=275, channels=2), FRAMES, FLOOR_WIDE),
    "w8192_h512": (dict(window_samples=8192, hop_samples=512, channels=2), FRAMES, FLOOR_K16),
    "w64_h16": (dict(window_samples=64, hop_samples=16, channels=2), FRAMES, FLOOR_WIDE),
    "w19200_large": (dict(window_samples=19200, hop_samples=4800, channels=2, large_transforms=True), 5, FLOOR_WIDE),
    "w32768_large": (dict(window_samples=32768, hop_samples=8192, channels=2, large_transforms=True), 3, FLOOR_WIDE),
}


def groups_of(frames):
    return [1, 5, 32, 33, 70, frames, frames + 10, SIZE_MAX]


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def make(name, **extra):
    return SpectrogramEngine(SR, device=0, **dict(CASES[name][0], **extra))


def noise(eng, frames, seed=0x5EED0D5D):
    """the engine's white noise: channel c is the stream of seed + c"""
    return eng.white_noise(eng.W + (frames - 1) * eng.H, seed=seed)


def spec_rows(eng, pcm, **kw):
    """sgx_stft_batch_complex as float32 words: [frames][pairs][M][2][2]"""
    import torch

    return torch.view_as_real(eng.stft_batch_complex(pcm, **kw)).contiguous()


KINDS = ("psd", "csd")


def kinds_of(eng):
    return KINDS if eng.channels >= 2 else ("psd",)


def batch(eng, kind, pcm, group, **kw):
    return eng.psd_batch(pcm, group, **kw) if kind == "psd" else eng.csd_batch(pcm, group, **kw)


@functools.lru_cache(maxsize=None)
def context(name):
    """one engine per case with its noise, its rows on the device, the summands x of the definition on the host, and the host reference
    of every group: computed once, shared by the tests, never written to"""
    import torch

    eng = make(name)
    frames = CASES[name][1]
    pcm = noise(eng, frames)
    mags, spec = eng.stft_batch(pcm), spec_rows(eng, pcm)
    torch.cuda.synchronize()
    x = {"psd": ref.psd_terms(mags.cpu().numpy()), "csd": ref.csd_terms(spec.cpu().numpy())}
    want = {(kind, g): ref.welch_mean(x[kind], g) for kind in KINDS for g in groups_of(frames)}
    for a in list(x.values()) + list(want.values()):
        a.setflags(write=False)
    return eng, pcm, {"psd": mags, "csd": spec}, x, want


# ---- 1: the batch calls, the stage calls and the host reference, bit for bit; counts; guards; the float64 bound ------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_counts_and_bound(name):
    import torch

    eng, pcm, rows, x, want = context(name)
    frames = CASES[name][1]
    assert eng.psd_fused == 0 and eng.csd_fused == 0
    for kind in kinds_of(eng):
        comps = 2 if kind == "psd" else 4
        # the float64 products of the same float32 rows, and the absolute products of each term
        if kind == "psd":
            x64 = rows[kind].cpu().numpy().astype(np.float64) ** 2
            a64 = x64
        else:
            x64, a64 = ref.csd_terms64(rows[kind].cpu().numpy())
        for g in groups_of(frames):
            expect = want[kind, g]
            cols = -(-frames // min(g, frames))
            assert expect.shape == (cols, eng.pairs, eng.M, comps)
            buf = torch.full((cols + 1, eng.pairs, eng.M, comps), float("nan"), dtype=torch.float32, device=eng.device)
            stale = bits(buf[cols:])
            batch(eng, kind, pcm, g, out=buf)                                     # (asserts *n_out == cols)
            staged = eng.psd_mags(rows[kind], g) if kind == "psd" else eng.csd_spec(rows[kind], g)
            torch.cuda.synchronize()
            assert np.array_equal(bits(buf[cols:]), stale), f"{name}/{kind}/{g}: bytes beyond n_out columns were written"
            assert np.array_equal(bits(buf[:cols]), expect.reshape(-1).view(np.uint32)), f"{name}/{kind}/{g}: not the host reference's bits"
            assert np.array_equal(bits(staged), bits(buf[:cols])), f"{name}/{kind}/{g}: the stage call differs from the batch call"
            mean, mean_abs = ref.mean64(x64, g), ref.mean64(a64, g)
            err = np.abs(buf[:cols].cpu().numpy().astype(np.float64) - mean)
            allow = BOUND * mean_abs
            worst = float((err / np.maximum(allow, 1e-300)).max())
            print(f"{name}/{kind}/group {g}: worst |got - float64| / bound = {worst:.3f}")
            assert (err <= allow).all(), f"{name}/{kind}/{g}: {worst:.3f} x the 35 * 2^-24 bound"
        # group = 1 is the summand itself
        one = batch(eng, kind, pcm, 1)
        assert np.array_equal(bits(one), (x[kind] + np.float32(0.0)).reshape(-1).view(np.uint32)), f"{name}/{kind}: group 1 is not x"
        # the last column is short where the group does not divide the frames
        if frames > 33:
            g = 33
            tail = batch(eng, kind, pcm, g, first_frame=(frames // g) * g)
            assert tail.shape[0] == 1 and np.array_equal(bits(tail), want[kind, g][-1].reshape(-1).view(np.uint32))
    # mono holds (v, v) wherever the rows do: every real-input route (the literal (s, s) transform of SGX_FLAG_COMPLEX_MONO rounds its two
    # sides apart, and paired frames hold what the rows hold)
    m = rows["psd"].cpu().numpy().view(np.uint32)
    if name == "w2048_h256_mono":
        assert np.array_equal(m[..., 0], m[..., 1])
    if eng.channels == 1 and np.array_equal(m[..., 0], m[..., 1]):
        v = batch(eng, "psd", pcm, 33).cpu().numpy().view(np.uint32)
        assert np.array_equal(v[..., 0], v[..., 1]), f"{name}: a mono stream does not hold (v, v)"


# ---- 2: a call split at column boundaries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_calls_equal_one_call(name):
    import torch

    eng, pcm, _, _, want = context(name)
    frames = CASES[name][1]
    g = 5 if frames >= 30 else (2 if frames >= 5 else 1)
    for kind in kinds_of(eng):
        full = batch(eng, kind, pcm, g)
        cols = full.shape[0]
        for cuts in ([cols // 3], [cols // 3, 2 * cols // 3]):
            edges = [0] + [c * g for c in cuts] + [frames]
            parts = [batch(eng, kind, pcm, g, first_frame=a, max_frames=b - a) for a, b in zip(edges[:-1], edges[1:])]
            torch.cuda.synchronize()
            assert sum(p.shape[0] for p in parts) == cols
            assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(full)), f"{name}/{kind}: split at frames {edges}"
    if frames > 40:                                                               # a split inside the long group's second block boundary
        for kind in kinds_of(eng):
            a, b = batch(eng, kind, pcm, 33, max_frames=33), batch(eng, kind, pcm, 33, first_frame=33)
            assert np.array_equal(np.concatenate([bits(a), bits(b)]), want[kind, 33].reshape(-1).view(np.uint32))


# ---- 3: end to end against the float64 truth -------------------------------------------------------------------------------------------
def carried_allowance(L, R, floor):
    """the rows' own allowance e = REL_TOL max(|ref|, floor peak) per bin and side, carried through the products: [..., M] complex128
    truths -> the allowances of psd [..., M, 2] and of csd [..., M, 4]"""
    aL, aR = np.abs(L), np.abs(R)
    peak = np.maximum(aL.max(axis=-1, keepdims=True), aR.max(axis=-1, keepdims=True))
    eL, eR = REL_TOL * np.maximum(aL, floor * peak), REL_TOL * np.maximum(aR, floor * peak)
    sq = np.stack([2.0 * aL * eL + eL * eL, 2.0 * aR * eR + eR * eR], -1)
    mixed = aL * eR + aR * eL + eL * eR
    return sq, np.concatenate([sq, np.stack([mixed, mixed], -1)], -1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_float64_truth(name):
    eng, pcm, rows, _, _ = context(name)
    frames, floor = CASES[name][1], CASES[name][2]
    samples = pcm.cpu().numpy().reshape(-1, eng.channels)
    for g in (33, SIZE_MAX):
        got = {kind: batch(eng, kind, pcm, g).cpu().numpy().astype(np.float64) for kind in kinds_of(eng)}
        for pair in range(eng.pairs):
            lr = samples[:, [0, 0]] if eng.channels == 1 else samples[:, 2 * pair:2 * pair + 2]
            t = np.stack([truth_complex(lr[f * eng.H:f * eng.H + eng.W], eng.W) for f in range(frames)])     # [frames][M][2] complex128
            L, R = t[..., 0], t[..., 1]
            z = L * np.conj(R)
            truth4 = np.stack([np.abs(L) ** 2, np.abs(R) ** 2, z.real, z.imag], -1)
            cross = np.abs(L) * np.abs(R)                                         # |a c| + |b d| and |b c| + |a d| are at most |L| |R|
            abs4 = np.stack([np.abs(L) ** 2, np.abs(R) ** 2, cross, cross], -1)
            allow2, allow4 = carried_allowance(L, R, floor)
            for kind in kinds_of(eng):
                truth, allow, mag = (truth4[..., :2], allow2, abs4[..., :2]) if kind == "psd" else (truth4, allow4, abs4)
                bound = ref.mean64(allow, g) + BOUND * ref.mean64(mag + allow, g)
                err = np.abs(got[kind][:, pair] - ref.mean64(truth, g))
                worst = float((err / bound).max())
                print(f"{name}/{kind}/group {g} pair {pair}: worst |got - truth| / allowance = {worst:.3f}")
                assert (err <= bound).all(), f"{name}/{kind}/{g} pair {pair}: {worst:.3f} x the allowance"


# ---- 4: a sinusoid at a bin centre: the scaling the header states ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr", "w2400_h93_lr", "w64_h16", "w8192_h512"])
def test_sinusoid_at_a_bin_centre(name):
    import torch

    eng = context(name)[0]
    W, frames = eng.W, 40
    n = W + (frames - 1) * eng.H
    tone = (0.5 * np.cos(0.5 * np.pi * np.arange(n))).astype(np.float32)           # bin W / 2 of the 2W-point transform; 0.5, 0, -0.5, 0 exactly
    pcm = torch.from_numpy(np.repeat(tone[:, None], eng.channels, 1).reshape(-1).copy()).to(eng.device)
    m = 0.5 * float(eng.window().astype(np.float64).sum()) / W
    e = REL_TOL * m
    allow = 2.0 * m * e + e * e + BOUND * (m + e) ** 2
    j = W // 2 - 1                                                                # stored element j is bin j + 1
    for g in groups_of(frames):
        psd = eng.psd_batch(pcm, g).cpu().numpy().astype(np.float64)[:, :, j]
        worst = float(np.abs(psd - m * m).max() / allow)
        print(f"{name}/psd/group {g}: worst |got - (A S1 / W)^2| / allowance = {worst:.3f}")
        assert worst <= 1.0, f"{name}/psd/{g}"
        if eng.channels >= 2:
            csd = eng.csd_batch(pcm, g).cpu().numpy().astype(np.float64)[:, :, j]
            assert (np.abs(csd[..., :3] - m * m) <= allow).all() and (np.abs(csd[..., 3]) <= allow).all(), f"{name}/csd/{g}"


# ---- 5: the seams of the workspace's ranges -----------------------------------------------------------------------------------------------
def test_range_seam_at_w2048_ch8():
    """8 channels: a row and a block partial are 64 KB each, 3073 of either fit the workspace.  group 1 takes 1536 frames per range, group 3
    768 columns (2304 frames): both calls cross a seam, and are compared on the device"""
    import torch

    eng = context("w2048_ch8")[0]
    cap = WORKSPACE_BYTES // (eng.pairs * eng.M * 2 * 4)
    frames = 2400
    assert frames > cap // 2 and frames > 3 * (cap // 4)
    pcm = noise(eng, frames, seed=77)
    mags = eng.stft_batch(pcm)
    x = mags * mags
    one = eng.psd_batch(pcm, 1)
    assert torch.equal(one.view(torch.int32), x.view(torch.int32)), "group 1 across the seam is not rn(m * m)"
    seam = cap // 2
    parts = [eng.psd_batch(pcm, 1, max_frames=seam), eng.psd_batch(pcm, 1, first_frame=seam)]
    assert torch.equal(torch.cat(parts).view(torch.int32), one.view(torch.int32))
    del one, parts
    three = eng.psd_batch(pcm, 3)
    t = x.view(frames // 3, 3, eng.pairs, eng.M, 2)
    s = (t[:, 0] + t[:, 1]) + t[:, 2]                                             # the float32 chain of a block of three frames
    expect = (s.double() / 3.0).float()
    assert torch.equal(three.view(torch.int32), expect.view(torch.int32)), "group 3 across the seam"
    seam = 3 * (cap // 4)
    parts = [eng.psd_batch(pcm, 3, max_frames=seam), eng.psd_batch(pcm, 3, first_frame=seam)]
    assert torch.equal(torch.cat(parts).view(torch.int32), three.view(torch.int32))
    torch.cuda.synchronize()


def strided_reference(kind, rows, group, stride):
    bins = rows[:, :, ::stride].cpu().numpy()
    return ref.welch_mean(ref.psd_terms(bins) if kind == "psd" else ref.csd_terms(bins), group)


@pytest.mark.parametrize("kind", KINDS)
def test_ranges_shorter_than_the_call_at_w19200(kind):
    """W 19200 with 8 channels: 327 rows (163 complex rows) fit the workspace, the call has 400 frames.  Group 33 takes several ranges of
    whole columns; one column of 400 frames has more blocks than a range holds and is carried in the float64 row"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=19200, hop_samples=4800, channels=8, large_transforms=True)
    frames, stride = 400, 64
    cap = WORKSPACE_BYTES // (eng.pairs * eng.M * (8 if kind == "psd" else 16))
    assert cap // 33 < -(-frames // 32) and cap < frames
    pcm = noise(eng, frames, seed=5)
    rows = eng.stft_batch(pcm) if kind == "psd" else spec_rows(eng, pcm)
    for g in (33, 100, SIZE_MAX):
        got = batch(eng, kind, pcm, g)
        staged = eng.psd_mags(rows, g) if kind == "psd" else eng.csd_spec(rows, g)
        assert np.array_equal(bits(got), bits(staged)), f"{kind}/{g}: batch and stage"
        want = strided_reference(kind, rows, g, stride)
        assert np.array_equal(bits(got[:, :, ::stride]), want.reshape(-1).view(np.uint32)), f"{kind}/{g}: not the host reference's bits"
        if g != SIZE_MAX:
            cut = (got.shape[0] // 2) * g
            parts = [batch(eng, kind, pcm, g, max_frames=cut), batch(eng, kind, pcm, g, first_frame=cut)]
            assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(got)), f"{kind}/{g}: split at frame {cut}"
    torch.cuda.synchronize()
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_rows_too_long_for_a_block_at_w32768_ch64(kind):
    """W 32768 with 64 channels: 24 rows (12 complex rows) fit the workspace -- fewer than a block of 32 frames and its partial row.  The
    batch call takes a block's rows a few frames at a time and continues the block's chain; the bits stay the definition's"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=32768, hop_samples=8192, channels=64, large_transforms=True)
    frames, stride = 36, 512
    cap = WORKSPACE_BYTES // (eng.pairs * eng.M * (8 if kind == "psd" else 16))
    assert 2 <= cap < 33
    pcm = noise(eng, frames, seed=9)
    rows = eng.stft_batch(pcm) if kind == "psd" else spec_rows(eng, pcm)
    for g in (33, SIZE_MAX, 5):
        got = batch(eng, kind, pcm, g)
        want = strided_reference(kind, rows, g, stride)
        assert np.array_equal(bits(got[:, :, ::stride]), want.reshape(-1).view(np.uint32)), f"{kind}/{g}: not the host reference's bits"
        staged = eng.psd_mags(rows, g) if kind == "psd" else eng.csd_spec(rows, g)
        assert np.array_equal(bits(got), bits(staged)), f"{kind}/{g}: batch and stage"
    torch.cuda.synchronize()
    eng.close()


# ---- 6: compute-unit limits and streams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr", "w2048_ch4", "w2400_h93_lr", "w8192_h512"])
def test_cu_limits_and_streams(name):
    import torch

    eng, pcm, _, _, want = context(name)
    try:
        for kind in kinds_of(eng):
            for g in (33, 5):
                expect = want[kind, g].reshape(-1).view(np.uint32)
                for limit in (1, 3, 0):
                    eng.set_cu_limit(limit)
                    assert np.array_equal(bits(batch(eng, kind, pcm, g)), expect), f"{name}/{kind}/{g}: {limit} CUs"
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):                                        # (the engine binds to torch's current stream)
                    other = batch(eng, kind, pcm, g)
                s.synchronize()
                assert np.array_equal(bits(other), expect), f"{name}/{kind}/{g}: a non-default stream"
    finally:
        eng.set_cu_limit(0)
        eng.use_current_stream()
    torch.cuda.synchronize()


# ---- 7: arguments -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_lr", "w2400_h93_lr", "w64_h16"])
def test_arguments(name):
    import torch

    eng, pcm, rows, _, want = context(name)
    frames = CASES[name][1]
    n = pcm.numel() // eng.channels
    lib, got = eng._lib, C.c_size_t(7)
    vp = lambda t: C.c_void_p(t.data_ptr())
    bad = _lib.SGX_ERR_INVALID_ARG
    words = frames * eng.pairs * eng.M * 4
    buf = torch.full((words + 8,), float("nan"), dtype=torch.float32, device=eng.device)
    stale = bits(buf)
    for fn, who in ((lib.sgx_psd_batch, b"sgx_psd_batch"), (lib.sgx_csd_batch, b"sgx_csd_batch")):
        assert fn(eng._ctx, vp(pcm), n, 0, 1000, 0, vp(buf), C.byref(got)) == bad and got.value == 0      # group 0
        assert who in lib.sgx_last_error(eng._ctx)
        got = C.c_size_t(7)
        assert fn(eng._ctx, None, n, 0, 1000, 5, vp(buf), C.byref(got)) == bad and got.value == 0
        assert fn(eng._ctx, vp(pcm), n, 0, 1000, 5, None, C.byref(got)) == bad
        assert fn(None, vp(pcm), n, 0, 1000, 5, vp(buf), C.byref(got)) == bad
        got = C.c_size_t(7)
        assert fn(eng._ctx, vp(pcm), eng.W - 1, 0, 10, 5, vp(buf), C.byref(got)) == 0 and got.value == 0  # too few samples
        assert fn(eng._ctx, vp(pcm), n, frames, 10, 5, vp(buf), C.byref(got)) == 0 and got.value == 0     # no frame in range
        assert fn(eng._ctx, vp(pcm), n, 0, 1000, 5, vp(buf), None) == 0                                   # n_out may be null
    for fn, who, r in ((lib.sgx_psd_mags, b"sgx_psd_mags", rows["psd"]), (lib.sgx_csd_spec, b"sgx_csd_spec", rows["csd"])):
        got = C.c_size_t(7)
        assert fn(eng._ctx, vp(r), frames, 0, vp(buf), C.byref(got)) == bad and got.value == 0
        assert who in lib.sgx_last_error(eng._ctx)
        assert fn(eng._ctx, None, frames, 5, vp(buf), C.byref(got)) == bad
        assert fn(eng._ctx, vp(r), frames, 5, None, C.byref(got)) == bad
        assert fn(None, vp(r), frames, 5, vp(buf), C.byref(got)) == bad
        got = C.c_size_t(7)
        assert fn(eng._ctx, vp(r), 0, 5, vp(buf), C.byref(got)) == 0 and got.value == 0
    assert lib.sgx_psd_fused(None) == bad and lib.sgx_csd_fused(None) == bad
    # a misaligned csd buffer: refused, nothing written
    torch.cuda.synchronize()
    buf.fill_(float("nan"))
    off = C.c_void_p(buf.data_ptr() + 4)
    got = C.c_size_t(7)
    assert lib.sgx_csd_batch(eng._ctx, vp(pcm), n, 0, 1000, 5, off, C.byref(got)) == bad and got.value == 0
    assert b"aligned" in lib.sgx_last_error(eng._ctx)
    assert lib.sgx_csd_spec(eng._ctx, vp(rows["csd"]), frames, 5, off, C.byref(got)) == bad
    assert lib.sgx_csd_spec(eng._ctx, C.c_void_p(rows["csd"].data_ptr() + 4), frames - 1, 5, vp(buf), C.byref(got)) == bad
    torch.cuda.synchronize()
    assert np.array_equal(bits(buf), stale), f"{name}: a refused call wrote to its buffer"
    # psd needs no more than the rows' own 8-byte alignment
    eng._check(lib.sgx_psd_batch(eng._ctx, vp(pcm), n, 0, 1000, 33, C.c_void_p(buf.data_ptr() + 8), C.byref(got)))
    torch.cuda.synchronize()
    cols = want["psd", 33].shape[0]
    assert got.value == cols
    assert np.array_equal(bits(buf[2:2 + want["psd", 33].size]), want["psd", 33].reshape(-1).view(np.uint32))


def test_mono_context():
    import torch

    eng, pcm, rows, _, _ = context("w2048_h256_mono")
    out = torch.zeros(FRAMES * eng.M * 4, dtype=torch.float32, device=eng.device)
    got = C.c_size_t(7)
    rc = eng._lib.sgx_csd_batch(eng._ctx, C.c_void_p(pcm.data_ptr()), pcm.numel(), 0, FRAMES, 5, C.c_void_p(out.data_ptr()), C.byref(got))
    assert rc == _lib.SGX_ERR_UNSUPPORTED and got.value == 0
    assert b"sgx_csd_batch" in eng._lib.sgx_last_error(eng._ctx)
    torch.cuda.synchronize()
    assert not out.any()
    # the stage serves the mono rows: (X, X) per bin, so x0 == x1 == x2 and x3 == +0.0
    for g in (1, 33):
        v = eng.csd_spec(rows["csd"], g).cpu().numpy().view(np.uint32)
        assert np.array_equal(v[..., 0], v[..., 1]) and np.array_equal(v[..., 0], v[..., 2]) and (v[..., 3] == 0).all()


def test_stream_ordered_and_asynchronous():
    """queued behind a long kernel on a non-default stream, the call returns before that kernel ends; the input is written on the same
    stream behind the sleep, so work put anywhere else would read NaN"""
    import torch

    for name in ["w2048_h256_lr", "w8192_h512"]:
        eng = make(name)
        n = eng.W + (FRAMES - 1) * eng.H
        refs = [eng.psd_batch(eng.white_noise(n, seed=21), 33), eng.csd_batch(eng.white_noise(n, seed=21), 33)]   # (the workspace is grown here)
        torch.cuda.synchronize()
        pcm = torch.full((n * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
        outs = [torch.full_like(r, -1.0) for r in refs]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        eng.set_stream(s.cuda_stream)
        lib, got = eng._lib, C.c_size_t(0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(400_000_000)
        eng._check(lib.sgx_synth_white_noise(eng._ctx, C.c_void_p(pcm.data_ptr()), 0, n, eng.channels, 21))
        eng._check(lib.sgx_psd_batch(eng._ctx, C.c_void_p(pcm.data_ptr()), n, 0, FRAMES, 33, C.c_void_p(outs[0].data_ptr()), C.byref(got)))
        eng._check(lib.sgx_csd_batch(eng._ctx, C.c_void_p(pcm.data_ptr()), n, 0, FRAMES, 33, C.c_void_p(outs[1].data_ptr()), C.byref(got)))
        done = torch.cuda.Event()
        done.record(s)
        assert not done.query(), f"{name}: the call waited for the stream"
        eng.sync()
        assert got.value == 3
        for out, r in zip(outs, refs):
            assert np.array_equal(bits(out), bits(r)), name
        eng.set_stream(0)
        eng.close()
