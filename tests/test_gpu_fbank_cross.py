"""sgx_fbank_cross_*: PCM to the per-band sums of |L|^2, |R|^2, Re L conj R and Im L conj R (include/sgx.h), through the C ABI.

The contract is that the output is a pure function of the frame's complex row and the bank: sgx_fbank_cross_batch -- one fused kernel at
W 2048 with 2 or 2k channels, the workspace route elsewhere -- equals sgx_fbank_cross_spec over sgx_stft_batch_complex's rows bit for bit,
on every transform family, sub-range, compute-unit limit and stream.  The values are held to the float64 sums over the engine's own
float32 rows within a derived bound: any path has at most 2 roundings in a product term, ceil(count / 64) in a lane's chain and 6 in the
tree, each relative 2^-24, plus one unit for the second-order terms: (ceil(count / 64) + 9) 2^-24 sum |w| m, m the sum of the absolute
products of the term.  End to end the sums are held to the float64 truth of the float32-windowed frame within the complex rows' own
allowance (tests/conftest.py) carried through the products.
(Every route runs one device body, so "bit-identical across routes" here compares that body with itself; tests/test_gpu_fbank_order.py
holds it to the header's products and sum order computed on the host, bit for bit.)"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import FLOOR_WIDE, PEAK_FLOOR, REL_TOL
from spectrogram_rs_amd import SpectrogramEngine, _lib
from test_gpu_complex import truth_complex
from test_gpu_fbank import dense, dense_over_limit, edges, mel128, pack, resized, unpack

pytestmark = pytest.mark.gpu

SR = 48000.0
FRAMES = 80
FUSED_MAX_WEIGHTS = 16384      # include/sgx.h: sgx_fbank_fused

_LR = dict(window_samples=2048, hop_samples=256, channels=2)
# name: (engine keyword arguments, frames, sgx_fbank_cross_fused for a bank within the stated size)
CASES = {
    "w2048_h256_lr": (_LR, FRAMES, 1),
    "w2048_h200_lr": (dict(window_samples=2048, hop_samples=200, channels=2), FRAMES, 1),
    "w2048_ch4": (dict(window_samples=2048, hop_samples=256, channels=4), FRAMES, 1),
    "w2048_ch8": (dict(window_samples=2048, hop_samples=256, channels=8), FRAMES, 1),
    "w2048_h256_lr_unfused": (dict(_LR, fused_render=False), FRAMES, 0),
    "w2048_h256_lr_generic": (dict(_LR, force_generic=True), FRAMES, 0),
    "w2400_h93_lr": (dict(window_samples=2400, hop_samples=93, channels=2), FRAMES, 0),
    "w1024_h256_lr": (dict(window_samples=1024, hop_samples=256, channels=2), FRAMES, 0),
    "w1102_chirpz": (dict(window_samples=1102, hop_samples=275, channels=2), FRAMES, 0),
    "w8192_h512": (dict(window_samples=8192, hop_samples=512, channels=2), FRAMES, 0),
    "w64_h16": (dict(window_samples=64, hop_samples=16, channels=2), FRAMES, 0),
    "w19200_large": (dict(window_samples=19200, hop_samples=4800, channels=2, large_transforms=True), 5, 0),
    # a column of 512 KB: no LDS holds it, the stage kernel reads the rows where they lie
    "w32768_large": (dict(window_samples=32768, hop_samples=8192, channels=2, large_transforms=True), 3, 0),
}
FUSED_CASES = [n for n, c in CASES.items() if c[2] == 1]


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def make(name, **extra):
    return SpectrogramEngine(SR, device=0, **dict(CASES[name][0], **extra))


def noise(eng, frames, seed=0x5EED0F0B):
    """the engine's white noise: channel c is the stream of seed + c"""
    return eng.white_noise(eng.W + (frames - 1) * eng.H, seed=seed)


def bank_of(kind, eng):
    return mel128(eng.W) if kind == "mel128" else edges(eng.M)


def rows_of(eng, pcm):
    """sgx_stft_batch_complex as float32 words: [frames][pairs][M][2][2] = (L.re, L.im), (R.re, R.im)"""
    import torch

    return torch.view_as_real(eng.stft_batch_complex(pcm)).contiguous()


def stage(fb, eng, rows):
    return fb.cross_apply(rows.reshape(-1, eng.M, 2, 2))


# ---- references ------------------------------------------------------------------------------------------------------------------
def products64(a, b, c, d):
    """x0 .. x3 of the definition in float64 and the sum m of the absolute products of each term, both [..., 4]"""
    x = np.stack([a * a + b * b, c * c + d * d, a * c + b * d, b * c - a * d], -1)
    m = np.stack([a * a + b * b, c * c + d * d, np.abs(a * c) + np.abs(b * d), np.abs(b * c) + np.abs(a * d)], -1)
    return x, m


def float64_sums(rows, bank):
    """rows [..., M, 2, 2] float32 -> (sum w x, the float32 allowance (ceil(count / 64) + 9) 2^-24 sum |w| m), both [..., n_filters, 4]"""
    r = rows.astype(np.float64)
    x, m = products64(r[..., 0, 0], r[..., 0, 1], r[..., 1, 0], r[..., 1, 1])
    d = dense(bank, rows.shape[-3])
    ref = np.einsum("fm,...mq->...fq", d, x)
    mag = np.einsum("fm,...mq->...fq", np.abs(d), m)
    steps = np.ceil(bank[1].astype(np.float64) / 64.0) + 9.0
    return ref, steps[:, None] * 2.0 ** -24 * mag


def check_against_rows(got, rows, bank, what):
    ref, allow = float64_sums(rows, bank)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(allow, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst |got - float64| / allowance = {worst:.3f}")
    assert (err <= allow).all(), f"{what}: {worst:.3f} x the float32 allowance"
    empty = bank[1] == 0
    if empty.any():
        assert (got[..., empty, :].view(np.uint32) == 0).all(), f"{what}: an empty filter is not four +0.0"


def products32(spec):
    """x0 .. x3 in numpy float32, every product and the one sum or difference rounded: [..., M, 2, 2] -> [..., M, 4]"""
    s = np.asarray(spec, np.float32)
    a, b, c, d = s[..., 0, 0], s[..., 0, 1], s[..., 1, 0], s[..., 1, 1]
    return np.stack([a * a + b * b, c * c + d * d, a * c + b * d, b * c - a * d], -1).astype(np.float32)


def carried(L, R, floor, bank):
    """the complex rows' own allowance e = REL_TOL max(|ref|, floor peak) per bin and side, carried through the four products and the
    bank: [..., M] complex128 truths -> [..., n_filters, 4]"""
    aL, aR = np.abs(L), np.abs(R)
    peak = np.maximum(aL.max(axis=-1, keepdims=True), aR.max(axis=-1, keepdims=True))
    eL, eR = REL_TOL * np.maximum(aL, floor * peak), REL_TOL * np.maximum(aR, floor * peak)
    mixed = aL * eR + aR * eL + eL * eR
    per_bin = np.stack([2.0 * aL * eL + eL * eL, 2.0 * aR * eR + eR * eR, mixed, mixed], -1)
    return np.einsum("fm,...mq->...fq", np.abs(dense(bank, L.shape[-1])), per_bin)


def truth_sums(L, R, bank):
    z = L * np.conj(R)
    x = np.stack([np.abs(L) ** 2, np.abs(R) ** 2, z.real, z.imag], -1)
    return np.einsum("fm,...mq->...fq", dense(bank, L.shape[-1]), x)


# ---- 1 + 2: routes bit for bit, and the values against the engine's own complex rows ------------------------------------------------
@pytest.mark.parametrize("kind", ["mel128", "edges"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_bit_for_bit_and_float64(name, kind):
    import torch

    eng = make(name)
    frames = CASES[name][1]
    pcm = noise(eng, frames)
    bank = bank_of(kind, eng)
    fb = eng.filterbank(*bank, power=2)
    assert fb.cross_fused == CASES[name][2], f"{name}/{kind}: sgx_fbank_cross_fused"
    got = fb.cross_batch(pcm)
    rows = rows_of(eng, pcm)
    staged = stage(fb, eng, rows).reshape(got.shape)
    from_complex64 = fb.cross_apply(eng.stft_batch_complex(pcm).reshape(-1, eng.M, 2))      # the rows as the engine hands them out
    torch.cuda.synchronize()
    assert np.array_equal(bits(from_complex64), bits(staged))
    assert got.shape == (frames, eng.pairs, fb.n_filters, 4)
    assert np.array_equal(bits(got), bits(staged)), f"{name}/{kind}: sgx_fbank_cross_batch differs from sgx_stft_batch_complex + sgx_fbank_cross_spec"
    if CASES[name][2]:
        split = make(name, fused_render=False)
        fb_split = split.filterbank(*bank, power=2)
        assert fb_split.cross_fused == 0
        other = fb_split.cross_batch(pcm)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), bits(other)), f"{name}/{kind}: fused and workspace routes differ"
        fb_split.close()
    # the bank's power plays no part
    fb1 = eng.filterbank(*bank, power=1)
    assert np.array_equal(bits(fb1.cross_batch(pcm)), bits(got)), f"{name}/{kind}: the power changed the cross sums"
    check_against_rows(got.cpu().numpy(), rows.cpu().numpy(), bank, f"{name}/{kind}")
    fb.close(), fb1.close()


# ---- 3: the stage's exact properties ----------------------------------------------------------------------------------------------
def synthetic_rows(columns, M, seed):
    """normal-range float32 values of either sign: magnitudes in [2^-10, 1)"""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.uniform(-10.0, 0.0, (columns, M, 2, 2)))
    return (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)


EXACT = {
    "w2048_h256_lr": CASES["w2048_h256_lr"][0],
    "w2400_h93_mono": dict(window_samples=2400, hop_samples=93),                       # the stage serves mono contexts like any other
    "w32768_large": CASES["w32768_large"][0],                                          # the rows read where they lie
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_stage_exact_properties(name):
    import torch

    eng = SpectrogramEngine(SR, device=0, **EXACT[name])
    M, columns = eng.M, 3
    spec = synthetic_rows(columns, M, 31)
    same = spec.copy()
    same[:, :, 1, :] = same[:, :, 0, :]                                                # R = L bitwise
    dev = lambda a: torch.from_numpy(a).to(eng.device)
    for kind in ("mel128", "edges"):
        bank = bank_of(kind, eng)
        fb = eng.filterbank(*bank, power=2)
        out = fb.cross_apply(dev(same)).cpu().numpy().view(np.uint32)
        assert out.shape == (columns, len(bank[0]), 4)
        assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2]), f"{name}/{kind}: L = R, yet out0, out1, out2 differ"
        assert (out[..., 3] == 0).all(), f"{name}/{kind}: L = R, yet out3 is not +0.0"
        check_against_rows(fb.cross_apply(dev(spec)).cpu().numpy(), spec, bank, f"{name}/{kind}/synthetic")
        fb.close()
    # single-bin filters of weight 1.0: one fused multiply-add by 1.0 from +0 and a tree of zeros are exact
    single = pack([(j, [1.0]) for j in range(M)])
    fb = eng.filterbank(*single, power=2)
    out = fb.cross_apply(dev(spec)).cpu().numpy()
    want = products32(spec) + np.float32(0.0)                                          # (x + 0: a -0.0 product term leaves the chain as +0.0)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), f"{name}: the products are not numpy float32's"
    fb.close()


# ---- 4: orientation and channel order by closed form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pair,floor", [("w2048_h256_lr", 0, PEAK_FLOOR), ("w2400_h93_lr", 0, FLOOR_WIDE), ("w2048_ch4", 1, PEAK_FLOOR)])
def test_orientation_by_closed_form(name, pair, floor):
    import torch

    eng = make(name)
    W, M, ch = eng.W, eng.M, eng.channels
    n0, d = W // 2, 3
    x = np.zeros((W, ch), np.float32)
    x[n0, 2 * pair], x[n0 + d, 2 * pair + 1] = 1.0, 1.0
    for other in range(eng.pairs):
        if other != pair:                                                              # the mirrored pair: the opposite phase
            x[n0 + d, 2 * other], x[n0, 2 * other + 1] = 1.0, 1.0
    win = eng.window().astype(np.float64)
    k = np.arange(1, W, dtype=np.float64)
    L = (2.0 / W) * win[n0] * np.exp(-1j * np.pi * k * n0 / W)
    R = (2.0 / W) * win[n0 + d] * np.exp(-1j * np.pi * k * (n0 + d) / W)
    z = L * np.conj(R)
    assert np.allclose(z, (2.0 / W) ** 2 * win[n0] * win[n0 + d] * np.exp(1j * np.pi * k * d / W), rtol=1e-12, atol=0.0)
    bank = pack([(0, [1.0]), (W // 4 - 1, [1.0]), (W - 2, [1.0]), (W // 2 - 33, np.ones(65))])     # bins k = 1, W / 4, W - 1; 65 unit weights
    fb = eng.filterbank(*bank, power=2)
    pcm = torch.from_numpy(x.reshape(-1)).to(eng.device)
    got = fb.cross_batch(pcm).cpu().numpy()
    rows = rows_of(eng, pcm).cpu().numpy()
    assert got.shape == (1, eng.pairs, 4, 4)
    ref = truth_sums(L, R, bank)
    _, rounding = float64_sums(rows[0, pair], bank)
    allow = carried(L, R, floor, bank) + rounding
    err = np.abs(got[0, pair].astype(np.float64) - ref)
    worst = float((err / allow).max())
    print(f"{name} pair {pair}: worst |got - closed form| / allowance = {worst:.3f}")
    assert (err <= allow).all(), f"{name} pair {pair}: {worst:.3f} x the allowance"
    # the check sees the orientation: the conjugate (or l and r swapped) misses the imaginary part by far more than the allowance
    assert (np.abs(ref[..., 3]) > 100.0 * allow[..., 3]).all()
    fb.close()


# ---- 5: end to end against the float64 truth ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,floor", [("w2048_h256_lr", PEAK_FLOOR), ("w2048_ch4", PEAK_FLOOR), ("w2400_h93_lr", FLOOR_WIDE)])
def test_against_the_float64_truth(name, floor):
    import torch

    eng = make(name)
    pcm = noise(eng, FRAMES)
    bank = mel128(eng.W)
    fb = eng.filterbank(*bank, power=2)
    got, rows = fb.cross_batch(pcm), rows_of(eng, pcm)
    torch.cuda.synchronize()
    got, rows = got.cpu().numpy(), rows.cpu().numpy()
    x = pcm.cpu().numpy().reshape(-1, eng.channels)
    worst = 0.0
    for pair in range(eng.pairs):
        lr = x[:, 2 * pair:2 * pair + 2]
        t = np.stack([truth_complex(lr[f * eng.H:f * eng.H + eng.W], eng.W) for f in range(FRAMES)])     # [frames][M][2] complex128
        L, R = t[..., 0], t[..., 1]
        _, rounding = float64_sums(rows[:, pair], bank)
        allow = carried(L, R, floor, bank) + rounding
        err = np.abs(got[:, pair].astype(np.float64) - truth_sums(L, R, bank))
        worst = max(worst, float((err / allow).max()))
        assert (err <= allow).all(), f"{name} pair {pair}: {float((err / allow).max()):.3f} x the allowance"
    print(f"{name}: worst |got - truth| / allowance = {worst:.3f}")
    fb.close()


# ---- 6: sub-ranges and seams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FUSED_CASES + ["w2400_h93_lr", "w8192_h512"])
def test_slices_equal_the_whole_call(name):
    import torch

    eng = make(name)
    pcm = noise(eng, FRAMES, seed=11)
    fb = eng.filterbank(*mel128(eng.W), power=2)
    full = fb.cross_batch(pcm)
    for first, count in [(0, 1), (1, 7), (13, 30), (FRAMES - 5, None), (FRAMES - 1, 100)]:
        part = fb.cross_batch(pcm, first_frame=first, max_frames=count)
        end = FRAMES if count is None else min(first + count, FRAMES)
        assert np.array_equal(bits(part), bits(full[first:end])), f"{name}: [{first}, {end})"
    torch.cuda.synchronize()
    fb.close()


@pytest.mark.parametrize("name", FUSED_CASES)
def test_cu_limits(name):
    """1 and 3 compute units: every persistent workgroup runs many transforms"""
    import torch

    eng = make(name)
    pcm = noise(eng, 79, seed=17)
    fb = eng.filterbank(*mel128(eng.W), power=2)
    assert fb.cross_fused == 1
    full = fb.cross_batch(pcm)
    torch.cuda.synchronize()
    for limit in (1, 3):
        eng.set_cu_limit(limit)
        assert np.array_equal(bits(fb.cross_batch(pcm)), bits(full)), f"{name}: {limit} CUs"
        part = fb.cross_batch(pcm, first_frame=1, max_frames=5)
        assert np.array_equal(bits(part), bits(full[1:6])), f"{name}: frames 1 .. 5 at {limit} CUs"
    eng.set_cu_limit(0)
    torch.cuda.synchronize()
    fb.close()


@pytest.mark.parametrize("name", FUSED_CASES)
def test_bank_past_the_fused_limit(name):
    """the workspace route's bits are the fused route's for the filters the two banks share"""
    import torch

    eng = make(name)
    pcm = noise(eng, 11)
    bank = dense_over_limit(eng.M)
    assert bank[2].size > FUSED_MAX_WEIGHTS
    n_prefix = FUSED_MAX_WEIGHTS // eng.M                                              # whole-spectrum filters: the prefix within 16384 weights
    prefix = pack(unpack(bank)[:n_prefix])
    assert 0 < n_prefix <= 1024 and prefix[2].size <= FUSED_MAX_WEIGHTS
    fb, fp = eng.filterbank(*bank, power=2), eng.filterbank(*prefix, power=2)
    assert fb.cross_fused == 0 and fp.cross_fused == 1
    got, short = fb.cross_batch(pcm), fp.cross_batch(pcm)
    rows = rows_of(eng, pcm)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got[:, :, :n_prefix]), bits(short)), f"{name}: the two routes differ on the shared filters"
    assert np.array_equal(bits(got), bits(stage(fb, eng, rows).reshape(got.shape)))
    check_against_rows(got.cpu().numpy(), rows.cpu().numpy(), bank, f"{name}/dense")
    fb.close(), fp.close()


@pytest.mark.parametrize("n_filters", [1, 63, 64, 65, 257, 1000])
def test_filter_counts(n_filters):
    import torch

    name = "w2048_h256_lr"
    eng = make(name)
    pcm = noise(eng, 9)
    bank = resized(edges(eng.M), n_filters)
    fb = eng.filterbank(*bank, power=2)
    assert fb.n_filters == n_filters
    assert fb.cross_fused == (1 if bank[2].size <= FUSED_MAX_WEIGHTS and n_filters <= 1024 else 0)
    got, rows = fb.cross_batch(pcm), rows_of(eng, pcm)
    staged = stage(fb, eng, rows).reshape(got.shape)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(staged))
    check_against_rows(got.cpu().numpy(), rows.cpu().numpy(), bank, f"{name}/edges x{n_filters}")
    fb.close()


# ---- 7: guards and contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_lr", "w2048_ch4", "w2400_h93_lr", "w64_h16"])
def test_guards_and_arguments(name):
    import torch

    eng = make(name)
    frames = 13
    n = eng.W + (frames - 1) * eng.H
    fb = eng.filterbank(*mel128(eng.W), power=2)
    clean = noise(eng, frames, seed=23)
    want = bits(fb.cross_batch(clean))
    pcm = torch.full(((n + 4096) * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
    pcm[:n * eng.channels] = clean
    words = frames * eng.pairs * fb.n_filters * 4
    guard, sentinel = 4096, 0x7FC0BEEF
    buf = torch.full((guard + words + guard,), float("nan"), dtype=torch.float32, device=eng.device)      # a stale output: every word NaN
    buf.view(torch.int32)[:guard] = sentinel
    buf.view(torch.int32)[guard + words:] = sentinel
    lib, got = eng._lib, C.c_size_t(0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    eng._check(lib.sgx_fbank_cross_batch(fb._h, vp(pcm), n, 0, 1000, C.c_void_p(buf.data_ptr() + 4 * guard), C.byref(got)))
    torch.cuda.synchronize()
    assert got.value == frames
    host = buf.cpu().numpy()
    assert (host[:guard].view(np.uint32) == sentinel).all() and (host[guard + words:].view(np.uint32) == sentinel).all()
    assert np.isfinite(host[guard:guard + words]).all(), f"{name}: a word of the output was not written"
    assert np.array_equal(host[guard:guard + words].view(np.uint32), want)
    # too few samples: no frame, and the buffer is not touched
    got = C.c_size_t(123)
    assert lib.sgx_fbank_cross_batch(fb._h, vp(pcm), eng.W - 1, 0, 10, C.c_void_p(buf.data_ptr() + 4 * guard), C.byref(got)) == 0
    torch.cuda.synchronize()
    assert got.value == 0 and np.array_equal(buf.cpu().numpy().view(np.uint32), host.view(np.uint32))
    bad = _lib.SGX_ERR_INVALID_ARG
    out = buf[guard:]
    assert lib.sgx_fbank_cross_batch(fb._h, None, n, 0, 10, vp(out), C.byref(got)) == bad
    assert b"sgx_fbank_cross_batch" in lib.sgx_last_error(eng._ctx)
    assert lib.sgx_fbank_cross_batch(fb._h, vp(pcm), n, 0, 10, None, C.byref(got)) == bad
    assert lib.sgx_fbank_cross_batch(None, vp(pcm), n, 0, 10, vp(out), C.byref(got)) == bad
    assert lib.sgx_fbank_cross_spec(fb._h, None, 1, vp(out)) == bad
    assert b"sgx_fbank_cross_spec" in lib.sgx_last_error(eng._ctx)
    assert lib.sgx_fbank_cross_spec(fb._h, vp(pcm), 1, None) == bad
    assert lib.sgx_fbank_cross_spec(None, vp(pcm), 1, vp(out)) == bad
    assert lib.sgx_fbank_cross_fused(None) == bad
    fb.close()


def test_mono_context_is_unsupported():
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=256)
    fb = eng.filterbank(*mel128(eng.W), power=2)
    assert fb.cross_fused == 0
    pcm = eng.white_noise(eng.W + 4 * eng.H, seed=3)
    out = torch.zeros(5 * fb.n_filters * 4, dtype=torch.float32, device=eng.device)
    got = C.c_size_t(7)
    rc = eng._lib.sgx_fbank_cross_batch(fb._h, C.c_void_p(pcm.data_ptr()), pcm.numel(), 0, 5, C.c_void_p(out.data_ptr()), C.byref(got))
    assert rc == _lib.SGX_ERR_UNSUPPORTED and got.value == 0
    assert b"sgx_fbank_cross_batch" in eng._lib.sgx_last_error(eng._ctx)
    torch.cuda.synchronize()
    assert not out.any()
    # the stage serves the mono rows: (X, X) per bin, so out0 == out1 == out2 and out3 == +0.0
    rows = rows_of(eng, pcm)
    sums = fb.cross_apply(rows.reshape(-1, eng.M, 2, 2)).cpu().numpy().view(np.uint32)
    assert np.array_equal(sums[..., 0], sums[..., 1]) and np.array_equal(sums[..., 0], sums[..., 2]) and (sums[..., 3] == 0).all()
    fb.close()


def test_bank_that_outlives_its_context():
    import torch

    eng = make("w2048_h256_lr")
    lib = eng._lib
    first, count, weights = mel128(eng.W)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    eng._check(lib.sgx_fbank_create(eng._ctx, len(first), p(first), p(count), p(weights), 2, C.byref(h)))
    pcm = noise(eng, 3)
    n = pcm.numel() // eng.channels
    out = torch.zeros(3 * len(first) * 4, dtype=torch.float32, device=eng.device)
    vp = lambda t: C.c_void_p(t.data_ptr())
    got = C.c_size_t(0)
    assert lib.sgx_fbank_cross_fused(h) == 1
    assert lib.sgx_fbank_cross_batch(h, vp(pcm), n, 0, 3, vp(out), C.byref(got)) == 0 and got.value == 3
    torch.cuda.synchronize()
    eng.close()                                                                          # sgx_destroy: the bank is detached
    bad = _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_fbank_cross_batch(h, vp(pcm), n, 0, 3, vp(out), C.byref(got)) == bad and got.value == 0
    assert lib.sgx_fbank_cross_spec(h, vp(pcm), 1, vp(out)) == bad
    assert lib.sgx_fbank_cross_fused(h) == bad
    lib.sgx_fbank_destroy(h)


def test_stream_ordered_and_asynchronous():
    """queued behind a long kernel on a non-default stream, the call returns before that kernel ends; the input is written on the
    same stream behind the sleep, so work put anywhere else would read NaN"""
    import torch

    for name in ["w2048_h256_lr", "w8192_h512"]:
        eng = make(name)
        n = eng.W + (FRAMES - 1) * eng.H
        fb = eng.filterbank(*mel128(eng.W), power=2)
        assert fb.cross_fused == CASES[name][2]
        ref = fb.cross_batch(eng.white_noise(n, seed=21))
        torch.cuda.synchronize()
        pcm = torch.full((n * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
        out = torch.full((FRAMES, eng.pairs, fb.n_filters, 4), -1.0, dtype=torch.float32, device=eng.device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        eng.set_stream(s.cuda_stream)
        lib, got = eng._lib, C.c_size_t(0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(400_000_000)
        eng._check(lib.sgx_synth_white_noise(eng._ctx, C.c_void_p(pcm.data_ptr()), 0, n, eng.channels, 21))
        eng._check(lib.sgx_fbank_cross_batch(fb._h, C.c_void_p(pcm.data_ptr()), n, 0, FRAMES, C.c_void_p(out.data_ptr()), C.byref(got)))
        done = torch.cuda.Event()
        done.record(s)
        assert not done.query(), f"{name}: sgx_fbank_cross_batch waited for the stream"
        eng.sync()
        assert got.value == FRAMES
        assert np.array_equal(bits(out), bits(ref)), name
        eng.set_stream(0)
        fb.close()
