"""sgx_fbank_*: PCM to the weighted sums of a filterbank over the bin magnitudes or powers (include/sgx.h), through the C ABI.

The contract is that a bank's output is a pure function of the frame's row and the bank: sgx_fbank_batch -- one fused kernel at W 2048, the
workspace route elsewhere -- equals sgx_fbank_mags over sgx_stft_batch's rows bit for bit, on every transform family, sub-range, frame
count, compute-unit limit and stream.  The values are held to the float64 sum over the engine's own float32 rows within the standard
bound of a float32 sum of `count` products in any order, (count + 2) 2^-24 sum |w| x^p, and end to end to the float64 truth of the
float32-windowed frame within the rows' own allowance (tests/conftest.py) carried through the bank.
(Every route runs one device body, so "bit-identical across routes" here compares that body with itself; tests/test_gpu_fbank_order.py
holds it to the header's sum order computed on the host, bit for bit.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_signals as es
from conftest import FLOOR_WIDE, PEAK_FLOOR, REL_TOL
from spectrogram_rs_amd import SpectrogramEngine, _lib, mel_weights

pytestmark = pytest.mark.gpu

SR = 48000.0
FRAMES = 80
FUSED_MAX_WEIGHTS = 16384      # include/sgx.h: sgx_fbank_fused

# name: (engine keyword arguments, frames, sgx_fbank_fused for a bank within the stated size)
CASES = {
    "w2048_h256_mono": (dict(window_samples=2048, hop_samples=256), FRAMES, 1),
    "w2048_h200_mono": (dict(window_samples=2048, hop_samples=200), FRAMES, 1),
    "w2048_h256_lr": (dict(window_samples=2048, hop_samples=256, channels=2), FRAMES, 1),
    "w2048_h200_lr": (dict(window_samples=2048, hop_samples=200, channels=2), FRAMES, 1),
    "w2048_ch4": (dict(window_samples=2048, hop_samples=256, channels=4), FRAMES, 1),
    "w2048_ch8": (dict(window_samples=2048, hop_samples=256, channels=8), FRAMES, 1),
    "w2048_h256_paired": (dict(window_samples=2048, hop_samples=256, paired_frames=True), FRAMES, 0),
    "w2048_h256_complex": (dict(window_samples=2048, hop_samples=256, complex_mono=True), FRAMES, 0),
    "w2400_h93_mono": (dict(window_samples=2400, hop_samples=93), FRAMES, 0),
    "w2400_h93_lr": (dict(window_samples=2400, hop_samples=93, channels=2), FRAMES, 0),
    "w1102_chirpz": (dict(window_samples=1102, hop_samples=275), FRAMES, 0),
    "w8192_h512": (dict(window_samples=8192, hop_samples=512), FRAMES, 0),
    "w19200_large": (dict(window_samples=19200, hop_samples=4800, large_transforms=True), 5, 0),
    "w64_h16_generic": (dict(window_samples=64, hop_samples=16), FRAMES, 0),
    # a column of 256 KB: no LDS holds it, the stage kernel reads it where it lies
    "w32768_large": (dict(window_samples=32768, hop_samples=8192, large_transforms=True), 3, 0),
}
FUSED_CASES = [n for n, c in CASES.items() if c[2] == 1]


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def make(name, **extra):
    return SpectrogramEngine(SR, device=0, **CASES[name][0], **extra)


def noise(eng, frames, seed=0x5EED0F0B):
    return eng.white_noise(eng.W + (frames - 1) * eng.H, seed=seed)


# ---- banks -----------------------------------------------------------------------------------------------------------------
def pack(filters):
    """[(first, weights)] -> (first, count, weights) as sgx_fbank_create takes them"""
    first = np.array([f for f, _ in filters], np.uint32)
    count = np.array([len(w) for _, w in filters], np.uint32)
    weights = np.concatenate([np.asarray(w, np.float32).reshape(-1) for _, w in filters] + [np.zeros(0, np.float32)])
    return first, count, weights


def unpack(bank):
    first, count, weights = bank
    off = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
    return [(int(first[f]), weights[off[f]:off[f + 1]]) for f in range(len(first))]


@functools.lru_cache(maxsize=None)
def mel128(W):
    return mel_weights(SR, W, 128, 0.0, SR / 2)


@functools.lru_cache(maxsize=None)
def edges(M):
    """single bins at both ends, all bins at 1 / M, an empty filter, two identical overlapping ones, 63 .. 257 bins from odd starts in
    descending order, alternating signs"""
    rng = np.random.default_rng(5)
    f = [(0, [1.0]), (M - 1, [1.0]), (0, np.full(M, 1.0 / M)), (M, [])]
    n_ov = min(100, M // 2)
    ov = (M // 3, rng.uniform(-1.0, 1.0, n_ov))
    f += [ov, ov]
    prev = M
    for n in (63, 64, 65, 255, 256, 257):
        start = min(prev - 2, (M - n - 1) // 2 * 2 + 1 if M - n >= 1 else -1)
        if start < 1:
            continue
        f.append((start, rng.uniform(0.0, 1.0, n)))
        prev = start
    n_alt = min(33, M - 5)
    f.append((5, [(-1.0) ** i * (0.5 + i / 64.0) for i in range(n_alt)]))
    return pack(f)


def resized(bank, n):
    """the bank cut or repeated to n filters"""
    f = unpack(bank)
    return pack([f[i % len(f)] for i in range(n)])


def dense_over_limit(M):
    """whole-spectrum filters, just enough of them to pass the fused limit"""
    n = FUSED_MAX_WEIGHTS // M + 1
    rng = np.random.default_rng(9)
    return pack([(0, rng.uniform(0.0, 1.0, M)) for _ in range(n)])


def bank_of(kind, eng):
    return mel128(eng.W) if kind == "mel128" else edges(eng.M)


def dense(bank, M):
    d = np.zeros((len(bank[0]), M))
    for i, (first, w) in enumerate(unpack(bank)):
        d[i, first:first + len(w)] = w
    return d


def float64_sums(rows, bank, power):
    """rows [..., M, 2] float32 -> (sum w x^p, its float32 allowance (count + 2) 2^-24 sum |w| x^p), both [..., n_filters, 2]"""
    d = dense(bank, rows.shape[-2])
    x = rows.astype(np.float64) ** power
    ref = np.einsum("fm,...mc->...fc", d, x)
    mag = np.einsum("fm,...mc->...fc", np.abs(d), x)
    return ref, (bank[1].astype(np.float64)[:, None] + 2.0) * 2.0 ** -24 * mag


def check_against_rows(got, rows, bank, power, what):
    ref, allow = float64_sums(rows, bank, power)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(allow, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst |got - float64| / allowance = {worst:.3f}")
    assert (err <= allow).all(), f"{what}: {worst:.3f} x the float32 allowance"
    empty = bank[1] == 0
    if empty.any():
        assert (got[..., empty, :].view(np.uint32) == 0).all(), f"{what}: an empty filter is not +0.0"


# ---- 1 + 2: routes bit for bit, and the values against the engine's own rows ------------------------------------------------------
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("kind", ["mel128", "edges"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_bit_for_bit_and_float64(name, kind, power):
    import torch

    eng = make(name)
    frames = CASES[name][1]
    pcm = noise(eng, frames)
    bank = bank_of(kind, eng)
    fb = eng.filterbank(*bank, power=power)
    assert fb.n_filters == len(bank[0])
    assert fb.fused == CASES[name][2], f"{name}/{kind}: sgx_fbank_fused"
    got = fb.batch(pcm)
    rows = eng.stft_batch(pcm)
    staged = fb.apply(rows.reshape(-1, eng.M, 2)).reshape(got.shape)
    torch.cuda.synchronize()
    assert got.shape == (frames, eng.pairs, fb.n_filters, 2)
    assert np.array_equal(bits(got), bits(staged)), f"{name}/{kind}/p{power}: sgx_fbank_batch differs from sgx_stft_batch + sgx_fbank_mags"
    split = make(name, fused_render=False)
    fb_split = split.filterbank(*bank, power=power)
    assert fb_split.fused == 0
    other = fb_split.batch(pcm)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(other)), f"{name}/{kind}/p{power}: fused and workspace routes differ"
    check_against_rows(got.cpu().numpy(), rows.cpu().numpy(), bank, power, f"{name}/{kind}/p{power}")
    fb.close(), fb_split.close()


@pytest.mark.parametrize("name", FUSED_CASES)
def test_bank_past_the_fused_limit_takes_the_workspace_route(name):
    import torch

    eng = make(name)
    pcm = noise(eng, 11)
    bank = dense_over_limit(eng.M)
    assert bank[2].size > FUSED_MAX_WEIGHTS
    fb = eng.filterbank(*bank, power=2)
    assert fb.fused == 0
    got, rows = fb.batch(pcm), eng.stft_batch(pcm)
    staged = fb.apply(rows.reshape(-1, eng.M, 2)).reshape(got.shape)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(staged))
    check_against_rows(got.cpu().numpy(), rows.cpu().numpy(), bank, 2, f"{name}/dense")


@pytest.mark.parametrize("n_filters", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr", "w2400_h93_mono"])
def test_filter_counts(name, n_filters):
    import torch

    eng = make(name)
    pcm = noise(eng, 9)
    bank = resized(edges(eng.M), n_filters)
    fb = eng.filterbank(*bank, power=2)
    assert fb.n_filters == n_filters
    assert fb.fused == (1 if CASES[name][2] and bank[2].size <= FUSED_MAX_WEIGHTS and n_filters <= 1024 else 0)
    got, rows = fb.batch(pcm), eng.stft_batch(pcm)
    staged = fb.apply(rows.reshape(-1, eng.M, 2)).reshape(got.shape)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(staged))
    check_against_rows(got.cpu().numpy(), rows.cpu().numpy(), bank, 2, f"{name}/edges x{n_filters}")


# ---- 3: end to end against the float64 truth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("name,floor", [("w2048_h256_mono", PEAK_FLOOR), ("w2048_h256_lr", PEAK_FLOOR), ("w2400_h93_mono", FLOOR_WIDE)])
def test_against_the_float64_truth(name, floor, power):
    import torch

    eng = make(name)
    pcm = noise(eng, FRAMES)
    bank = mel128(eng.W)
    fb = eng.filterbank(*bank, power=power)
    got, rows = fb.batch(pcm), eng.stft_batch(pcm)
    torch.cuda.synchronize()
    got, rows = got.cpu().numpy()[:, 0], rows.cpu().numpy()[:, 0]
    x = pcm.cpu().numpy().reshape(-1, eng.channels)
    lr = x if eng.channels == 2 else np.repeat(x, 2, axis=1)
    t = np.stack([es.truth_frame(lr[f * eng.H:f * eng.H + eng.W], eng.W) for f in range(FRAMES)])      # [frames][M][2]
    peak = np.abs(t).max(axis=(-1, -2), keepdims=True)
    a = REL_TOL * np.maximum(np.abs(t), floor * peak)                                                    # the rows' own allowance
    d = dense(bank, eng.M)
    ref = np.einsum("fm,nmc->nfc", d, t ** power)
    carried = np.einsum("fm,nmc->nfc", np.abs(d), a if power == 1 else 2.0 * np.abs(t) * a + a * a)
    _, rounding = float64_sums(rows, bank, power)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / (carried + rounding)).max())
    print(f"{name}/p{power}: worst |got - truth| / allowance = {worst:.3f}")
    assert (err <= carried + rounding).all(), f"{name}/p{power}: {worst:.3f} x the allowance"


# ---- 4: sub-ranges and arguments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_paired", "w2048_h200_lr", "w2400_h93_mono", "w8192_h512"])
def test_slicing_and_arguments(name):
    import torch

    eng = make(name)
    pcm = noise(eng, FRAMES, seed=11)
    fb = eng.filterbank(*mel128(eng.W), power=2)
    full = fb.batch(pcm)
    for first, count in [(0, 1), (1, 7), (13, 30), (FRAMES - 5, None), (FRAMES - 1, 100)]:
        part = fb.batch(pcm, first_frame=first, max_frames=count)
        end = FRAMES if count is None else min(first + count, FRAMES)
        assert np.array_equal(bits(part), bits(full[first:end])), f"{name}: [{first}, {end})"
    torch.cuda.synchronize()
    lib, got = eng._lib, C.c_size_t(123)
    out = torch.empty(4, dtype=torch.float32, device=eng.device)
    vp = lambda t: C.c_void_p(t.data_ptr())
    short = pcm[:(eng.W - 1) * eng.channels]
    assert lib.sgx_fbank_batch(fb._h, vp(short), eng.W - 1, 0, 10, vp(out), C.byref(got)) == 0
    assert got.value == 0
    n = pcm.numel() // eng.channels
    bad = _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_fbank_batch(fb._h, None, n, 0, 10, vp(out), C.byref(got)) == bad
    assert b"sgx_fbank_batch" in lib.sgx_last_error(eng._ctx)
    assert lib.sgx_fbank_batch(fb._h, vp(pcm), n, 0, 10, None, C.byref(got)) == bad
    assert lib.sgx_fbank_batch(None, vp(pcm), n, 0, 10, vp(out), C.byref(got)) == bad
    assert lib.sgx_fbank_mags(fb._h, None, 1, vp(out)) == bad
    assert b"sgx_fbank_mags" in lib.sgx_last_error(eng._ctx)
    assert lib.sgx_fbank_mags(fb._h, vp(pcm), 1, None) == bad
    assert lib.sgx_fbank_mags(None, vp(pcm), 1, vp(out)) == bad
    assert lib.sgx_fbank_fused(None) == bad and lib.sgx_fbank_filters(None) == 0
    lib.sgx_fbank_destroy(None)


def test_invalid_banks_are_refused():
    eng = make("w2048_h256_mono")
    lib, M, bad = eng._lib, eng.M, _lib.SGX_ERR_INVALID_ARG
    first, count, w = np.array([0, 5], np.uint32), np.array([3, 2], np.uint32), np.arange(5, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(n=2, f=first, c=count, ww=w, power=2, ctx=None, out=True):
        h = C.c_void_p()
        rc = lib.sgx_fbank_create(eng._ctx if ctx is None else ctx, n, None if f is None else p(f), None if c is None else p(c),
                                  None if ww is None else p(ww), power, C.byref(h) if out else None)
        if rc == 0:
            lib.sgx_fbank_destroy(h)
        else:
            assert not h.value
        return rc

    assert create() == 0
    for kw in (dict(f=None), dict(c=None), dict(ww=None), dict(n=0), dict(power=0), dict(power=3), dict(out=False),
               dict(f=np.array([0, M - 1], np.uint32)),                          # first + count = M + 1
               dict(f=np.array([0, 0xFFFFFFFF], np.uint32)),                     # first + count wraps 32 bits
               dict(c=np.array([3, M + 1], np.uint32), ww=np.zeros(M + 4, np.float32)),
               dict(ww=np.array([0, 1, np.nan, 3, 4], np.float32)), dict(ww=np.array([0, 1, 2, 3, np.inf], np.float32)),
               dict(ww=np.array([-np.inf, 1, 2, 3, 4], np.float32))):
        assert create(**kw) == bad, kw
        assert b"sgx_fbank_create" in lib.sgx_last_error(eng._ctx), kw
    assert lib.sgx_fbank_create(None, 2, p(first), p(count), p(w), 2, C.byref(C.c_void_p())) == bad
    assert create(f=np.array([0, M - 2], np.uint32)) == 0                        # first + count = M: the last bin


# ---- 5: frame counts and job splits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h200_mono", "w2048_h256_lr"])
def test_frame_counts_and_cu_limits(name):
    import torch

    eng = make(name)
    pcm = noise(eng, 79, seed=17)
    fb = eng.filterbank(*mel128(eng.W), power=2)
    assert fb.fused == 1
    full = fb.batch(pcm)
    torch.cuda.synchronize()
    own = eng.cu_limit
    for limit in (1, 2, 3, own):
        eng.set_cu_limit(limit)
        for frames in (1, 2, 3, 5, 79):
            part = fb.batch(pcm[:(eng.W + (frames - 1) * eng.H) * eng.channels])
            assert np.array_equal(bits(part), bits(full[:frames])), f"{name}: {frames} frames at {limit} CUs"
            odd = fb.batch(pcm, first_frame=1, max_frames=frames)      # an odd first frame: the mono kernel's pairs start inside the range
            assert np.array_equal(bits(odd), bits(full[1:1 + frames])), f"{name}: {frames} frames from frame 1 at {limit} CUs"
    eng.set_cu_limit(0)
    torch.cuda.synchronize()


# ---- 6: guards and stale state ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr", "w2048_ch4", "w2400_h93_mono", "w64_h16_generic"])
def test_guards_and_stale_state(name):
    import torch

    eng = make(name)
    frames = 13
    n = eng.W + (frames - 1) * eng.H
    bank_a, bank_b = mel128(eng.W), edges(eng.M)
    fa, fb = eng.filterbank(*bank_a, power=2), eng.filterbank(*bank_b, power=1)
    clean = noise(eng, frames, seed=23)
    want_a, want_b = bits(fa.batch(clean)), bits(fb.batch(clean))
    pcm = torch.full(((n + 4096) * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
    pcm[:n * eng.channels] = clean
    words = frames * eng.pairs * fa.n_filters * 2
    guard, sentinel = 4096, 0x7FC0BEEF
    buf = torch.full((guard + words + guard,), float("nan"), dtype=torch.float32, device=eng.device)
    buf.view(torch.int32)[:guard] = sentinel
    buf.view(torch.int32)[guard + words:] = sentinel
    lib, got = eng._lib, C.c_size_t(0)
    eng._check(lib.sgx_fbank_batch(fa._h, C.c_void_p(pcm.data_ptr()), n, 0, 1000, C.c_void_p(buf.data_ptr() + 4 * guard), C.byref(got)))
    torch.cuda.synchronize()
    assert got.value == frames
    host = buf.cpu().numpy()
    assert (host[:guard].view(np.uint32) == sentinel).all() and (host[guard + words:].view(np.uint32) == sentinel).all()
    assert np.isfinite(host[guard:guard + words]).all()
    assert np.array_equal(host[guard:guard + words].view(np.uint32), want_a)
    # another bank on the same context gives its own bits, and the first bank its first bits again
    assert np.array_equal(bits(fb.batch(clean)), want_b)
    assert np.array_equal(bits(fa.batch(clean)), want_a)
    fb.close()
    assert np.array_equal(bits(fa.batch(clean)), want_a)
    torch.cuda.synchronize()


# ---- 7: stream order ------------------------------------------------------------------------------------------------------------------------
def test_stream_ordered_and_asynchronous():
    """queued behind a long kernel on a non-default stream, the call returns before that kernel ends; the input is written on the
    same stream behind the sleep, so work put anywhere else would read NaN"""
    import torch

    for name in ["w2048_h256_mono", "w8192_h512"]:
        eng = make(name)
        n = eng.W + (FRAMES - 1) * eng.H
        fb = eng.filterbank(*mel128(eng.W), power=2)
        assert fb.fused == CASES[name][2]
        ref = fb.batch(eng.white_noise(n, seed=21))
        torch.cuda.synchronize()
        pcm = torch.full((n * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
        out = torch.full((FRAMES, eng.pairs, fb.n_filters, 2), -1.0, dtype=torch.float32, device=eng.device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        eng.set_stream(s.cuda_stream)
        lib, got = eng._lib, C.c_size_t(0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(400_000_000)
        eng._check(lib.sgx_synth_white_noise(eng._ctx, C.c_void_p(pcm.data_ptr()), 0, n, eng.channels, 21))
        eng._check(lib.sgx_fbank_batch(fb._h, C.c_void_p(pcm.data_ptr()), n, 0, FRAMES, C.c_void_p(out.data_ptr()), C.byref(got)))
        done = torch.cuda.Event()
        done.record(s)
        assert not done.query(), f"{name}: sgx_fbank_batch waited for the stream"
        eng.sync()
        assert got.value == FRAMES
        assert np.array_equal(bits(out), bits(ref)), name
        eng.set_stream(0)


# ---- 8: nothing else moved ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr"])
def test_nothing_else_moved(name):
    import torch

    eng = make(name, gradient="viridis")
    pcm = noise(eng, 31, seed=29)

    def snapshot():
        out = (bits(eng.bands_batch(pcm)), bits(eng.render_batch(pcm)), bits(eng.stft_batch(pcm)), eng.bands_fused, eng._query().render_path)
        torch.cuda.synchronize()
        return out

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]

    before = snapshot()
    fb = eng.filterbank(*mel128(eng.W), power=2)
    assert same(before, snapshot()), "creating a bank changed another call's output"
    fb.batch(pcm)
    fb.apply(eng.stft_batch(pcm).reshape(-1, eng.M, 2))
    assert same(before, snapshot()), "running a bank changed another call's output"
    fb.close()
    assert same(before, snapshot())
