"""sgx_istft_batch: PCM back from the complex (L, R) spectra of sgx_stft_batch_complex, on every transform route the inverse serves
(tests/edge_signals.py's route table without the kernel-11 rows, plus hops W/4, W/2, odd hops and hops beyond W).  Checks: the round trip
through stft_batch_complex on the interior samples; edited spectra (random bins, a band mask) against the float64 definition of
include/sgx.h; channel separation; bit-identical results however the sample range is split and on a repeated run; spectra past byte
2^32; the call's contract.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import edge_signals as es

pytestmark = pytest.mark.gpu

EXTRA = [
    es.Route("mixed_w2048_h512_lr", 2048, 512, 2, ("force_generic",)),      # W / 4
    es.Route("k1_lr_h1024", 2048, 1024, 2),                                    # W / 2
    es.Route("chirpz_w1102_h551_lr", 1102, 551, 2),                             # W / 2, chirp-z
    es.Route("mixed_w2400_h601_mono", 2400, 601, 1),                            # odd hop, mono
    es.Route("k16_mono_h2048", 8192, 2048, 1),                                  # W / 4, 2W = 16384
    es.Route("chirpz_w1852_h463_ch4", 1852, 463, 4),                            # odd hop, four channels, chirp-z
    es.Route("mixed_w9600_h2400_lr", 9600, 2400, 2),                            # 2W = 19 200: 17-20 ring slots per thread at 512 threads
    es.Route("mixed_w8820_h2205_mono", 8820, 2205, 1),                          # 0.2 s at 44.1 kHz
    es.Route("mixed_w10240_h2560_lr", 10240, 2560, 2),                          # 2W = 20 480: the largest composite length, all 160 KB of LDS
]
ROUTES = [r for r in es.ROUTES if r.kernel != 11] + EXTRA
ROW = {r.name: r for r in ROUTES}
NAMES = [r.name for r in ROUTES]
# hops beyond the window (gaps where no frame covers a sample) and the 2W = 16384 context: the definition and the splits
WIDE = [es.Route("gap_w256_h300_lr", 256, 300, 2), es.Route("gap_w1102_h1500_mono", 1102, 1500, 1),
        es.Route("k16_lr_h512_split", 8192, 512, 2)]
ROUND_TRIP_TOL = 2e-5
DEFINITION_TOL = 1e-5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def engine(r, **extra):
    from spectrogram_rs_amd import SpectrogramEngine
    return SpectrogramEngine(es.SR, device=0, **r.engine_kwargs(), **extra)


def definition(spec, W, H, win, channels):
    """include/sgx.h's definition in float64: spec complex [F][pairs][M][2] -> x [(F-1) H + W][channels], envelope [(F-1) H + W]"""
    F, pairs = spec.shape[0], spec.shape[1]
    P, N = 2 * W, (spec.shape[0] - 1) * H + W
    w = win.astype(np.float64)
    num = np.zeros((N, channels))
    env = np.zeros(N)
    even = (np.arange(W, P) % 2) == 0
    par = np.arange(W) % 2
    for t in range(F):
        env[t * H:t * H + W] += w * w
    for pair in range(pairs):
        for side in range(1 if channels == 1 else 2):
            A = np.zeros((F, P), np.complex128)
            A[:, 1:W] = spec[:, pair, :, side]
            g = W * np.fft.ifft(A, axis=1).real
            ce = -g[:, W:][:, even].mean(axis=1)
            co = -g[:, W:][:, ~even].mean(axis=1)
            f = g[:, :W] + np.where(par[None, :] == 1, co[:, None], ce[:, None])
            ch = 0 if channels == 1 else 2 * pair + side
            for t in range(F):
                num[t * H:t * H + W, ch] += w * f[t]
    x = np.where(env[:, None] > 0, num / np.where(env > 0, env, 1.0)[:, None], 0.0)
    return x, env


def local_peak(a, W):
    """max |a| over [n - W, n + W] and the channel pair per sample (a [N][ch] -> [N][ch]): one complex transform carries both channels
    of a pair, so its rounding scales with the pair's peak"""
    from numpy.lib.stride_tricks import sliding_window_view
    m = np.abs(a)
    if m.shape[1] >= 2:
        m = np.repeat(m.reshape(m.shape[0], -1, 2).max(axis=2), 2, axis=1)
    pad = np.pad(m, ((W, W), (0, 0)))
    return sliding_window_view(pad, 2 * W + 1, axis=0).max(axis=-1)


def interior_min_env(W, H, win):
    e = np.zeros(H)
    w = win.astype(np.float64) ** 2
    for j in range(0, W, H):
        e[:min(H, W - j)] += w[j:j + H]
    return e.min()


def check_definition(got, ref, env, W, H, win, tol=DEFINITION_TOL):
    """|d| <= tol * local peak * max(1, E_int / E(n)) where E(n) >= 1e-3 E_int; finite elsewhere, exactly 0 where E(n) = 0.
    Returns the worst ratio of |d| to its bound."""
    e_int = interior_min_env(W, H, win) if H <= W // 2 else 1e-3 * env.max()
    assert np.isfinite(got).all()
    zero = env == 0
    assert (got[zero] == 0.0).all(), "the output must be exactly 0 where the envelope is 0"
    ok = env >= 1e-3 * e_int
    bound = tol * np.maximum(local_peak(ref, W), 1e-30) * np.maximum(1.0, e_int / np.where(env > 0, env, 1.0))[:, None]
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    return float(ratio[ok].max()) if ok.any() else 0.0


def forward(torch, eng, pcm):
    dev = torch.from_numpy(np.ascontiguousarray(pcm, np.float32).reshape(-1)).cuda()
    return eng.stft_batch_complex(dev)


def _signals(r, rng):
    """(name, [N][channels] float32) streams of at least 12 frames"""
    F = max(12, -(-3 * r.W // r.H) + 6)
    N = (F - 1) * r.H + r.W
    out = [("noise", rng.standard_normal((N, r.channels)).astype(np.float32))]
    step = np.full((N, r.channels), 1e-3, np.float32)
    at = (F // 2) * r.H + r.H // 3
    step[at:] = 1.0
    step *= np.where(np.arange(N) % 2, 1.0, -1.0).astype(np.float32)[:, None]
    out.append(("step60dB", step))
    imp = np.zeros((N, r.channels), np.float32)
    t0 = F // 2
    offs = sorted({1, r.W - 1, *[o for o in es.structural_offsets(r) if 0 < o < r.W][:12]})
    for i, o in enumerate(offs):
        imp[(t0 - 1 + i % 3) * r.H + o, i % r.channels] = 1.0 + 0.25 * i
    out.append(("impulses", imp))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_round_trip(torch_cuda, name):
    torch = torch_cuda
    r = ROW[name]
    eng = engine(r)
    assert eng.istft_supported() == 1
    rng = np.random.default_rng(7)
    for sig, x in _signals(r, rng):
        spec = forward(torch, eng, x)
        F = spec.shape[0]
        y = eng.istft_batch(spec)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        assert y.shape == ((F - 1) * r.H + r.W, r.channels)
        lo, hi = r.W - 1, F * r.H
        if r.H > r.W // 2:   # the round trip is held on hops up to W / 2 (the envelope of larger hops dips towards 0)
            continue
        d = np.abs(y[lo:hi].astype(np.float64) - x[lo:hi])
        allow = ROUND_TRIP_TOL * np.maximum(local_peak(x.astype(np.float64), r.W)[lo:hi], 1e-30)
        worst = float((d / allow).max())
        print(f"{name} {sig}: worst {worst:.3f} of the round-trip bound")
        assert worst <= 1.0, (name, sig, worst)


@pytest.mark.parametrize("name", NAMES + [r.name for r in WIDE])
def test_edited_spectra_against_the_definition(torch_cuda, name):
    torch = torch_cuda
    r = ROW.get(name) or {w.name: w for w in WIDE}[name]
    eng = engine(r)
    win = eng.window()
    rng = np.random.default_rng(11)
    F = max(6, -(-2 * r.W // r.H) + 3)
    M = r.W - 1
    rand = (rng.standard_normal((F, r.pairs, M, 2)) + 1j * rng.standard_normal((F, r.pairs, M, 2))).astype(np.complex64)
    x = rng.standard_normal(((F - 1) * r.H + r.W, r.channels)).astype(np.float32)
    masked = forward(torch, eng, x).cpu().numpy()
    k = np.arange(1, r.W)
    masked = masked * ((k > r.W // 8) & (k < r.W // 3))[None, None, :, None]
    other = (rng.standard_normal((F, r.pairs, M)) + 1j * rng.standard_normal((F, r.pairs, M))).astype(np.complex64)
    for sig, spec in (("random bins", rand), ("band mask", masked.astype(np.complex64))):
        if r.channels == 1:   # a mono context reads the L half only: R holds data of its own, which must not reach the output
            spec = spec.copy()
            spec[..., 1] = other
        y = eng.istft_batch(torch.from_numpy(spec).cuda())
        torch.cuda.synchronize()
        ref, env = definition(spec, r.W, r.H, win, r.channels)
        worst = check_definition(y.cpu().numpy(), ref, env, r.W, r.H, win)
        print(f"{name} {sig}: worst {worst:.3f} of the definition bound")
        assert worst <= 1.0, (name, sig, worst)


@pytest.mark.parametrize("name", [n for n in NAMES if ROW[n].channels >= 2])
def test_channel_separation(torch_cuda, name):
    torch = torch_cuda
    r = ROW[name]
    eng = engine(r)
    F = max(8, -(-2 * r.W // r.H) + 4)
    N = (F - 1) * r.H + r.W
    for ch in (0, 1, r.channels - 1):
        x = np.zeros((N, r.channels), np.float32)
        x[(F // 2) * r.H + r.W // 3, ch] = 1.0
        y = eng.istft_batch(forward(torch, eng, x))
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        quiet = np.delete(y, ch, axis=1)
        assert np.abs(quiet).max() <= ROUND_TRIP_TOL, (name, ch, float(np.abs(quiet).max()))
        assert abs(y[(F // 2) * r.H + r.W // 3, ch] - 1.0) <= ROUND_TRIP_TOL


@pytest.mark.parametrize("name", ["k1_lr_h256", "k48_lr", "chirpz_w1852_lr", "bluestein_w23", "k16_mono_h512", "mixed_w2205_real",
                                  "k1_ch8"] + [r.name for r in WIDE])
def test_splits_are_bit_identical(torch_cuda, name):
    torch = torch_cuda
    r = ROW.get(name) or {w.name: w for w in WIDE}[name]
    eng = engine(r)
    rng = np.random.default_rng(5)
    F = max(40, -(-6 * r.W // r.H))
    x = rng.standard_normal(((F - 1) * r.H + r.W, r.channels)).astype(np.float32)
    spec = forward(torch, eng, x)
    N = (spec.shape[0] - 1) * r.H + r.W
    a, b = int(rng.integers(0, r.W)), N - int(rng.integers(0, r.W))
    whole = eng.istft_batch(spec, first_sample=a, max_samples=b - a).clone()
    again = eng.istft_batch(spec, first_sample=a, max_samples=b - a).clone()
    cuts = sorted({a, b, *[int(c) for c in rng.integers(a + 1, b, 6)]})
    parts = [eng.istft_batch(spec, first_sample=lo, max_samples=hi - lo).clone() for lo, hi in zip(cuts[:-1], cuts[1:])]
    torch.cuda.synchronize()
    joined = torch.cat(parts)
    assert torch.equal(whole.view(torch.int32), again.view(torch.int32))
    assert torch.equal(whole.view(torch.int32), joined.view(torch.int32))


def test_spectra_past_4_gib(torch_cuda):
    torch = torch_cuda
    r = es.Route("offsets", 64, 16, 2)
    eng = engine(r)
    win = eng.window()
    per_frame = r.pairs * (r.W - 1) * 16
    F = (1 << 32) // per_frame + 64
    spec = torch.empty((F, r.pairs, r.W - 1, 2, 2), dtype=torch.float32, device="cuda")
    torch.manual_seed(3)
    spec.normal_()
    assert spec.numel() * 4 > 1 << 32
    K = 8
    N = (F - 1) * r.H + r.W
    s0 = (F - K) * r.H + r.W - 1
    y = eng.istft_batch(spec, first_sample=s0)
    torch.cuda.synchronize()
    tail = torch.view_as_complex(spec[F - K:].contiguous()).cpu().numpy()
    del spec
    ref, env = definition(tail, r.W, r.H, win, r.channels)
    off = s0 - (F - K) * r.H
    assert y.shape == (N - s0, 2)
    worst = check_definition(y.cpu().numpy(), ref[off:], env[off:], r.W, r.H, win)
    assert worst <= 1.0, worst


def test_spectra_past_2_32_elements(torch_cuda):
    """the last samples of spectra whose float4 element index passes 2^32 (64 GiB): only the frames the range reads are filled"""
    torch = torch_cuda
    r = es.Route("elements", 64, 16, 2)
    eng = engine(r)
    win = eng.window()
    M, K = r.W - 1, 8
    F = (1 << 32) // M + 64
    need = F * r.pairs * M * 16
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need + (4 << 30):
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free HBM, {free / 2**30:.1f} GiB free")
    spec = torch.empty((F, r.pairs, M, 2, 2), dtype=torch.float32, device="cuda")
    torch.manual_seed(4)
    spec[F - K:].normal_()
    assert (F - 1) * r.pairs * M + M - 1 >= 1 << 32
    N = (F - 1) * r.H + r.W
    s0 = (F - K) * r.H + r.W - 1          # every frame that covers [s0, N) is one of the last K
    y = eng.istft_batch(spec, first_sample=s0)
    torch.cuda.synchronize()
    tail = torch.view_as_complex(spec[F - K:].contiguous()).cpu().numpy()
    del spec
    torch.cuda.empty_cache()
    ref, env = definition(tail, r.W, r.H, win, r.channels)
    off = s0 - (F - K) * r.H
    assert y.shape == (N - s0, 2)
    worst = check_definition(y.cpu().numpy(), ref[off:], env[off:], r.W, r.H, win)
    assert worst <= 1.0, worst


def test_contract(torch_cuda):
    torch = torch_cuda
    from spectrogram_rs_amd import _lib
    r = es.ROUTE["k1_lr_h256"]
    eng = engine(r)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((9 * r.H + r.W, 2)).astype(np.float32)
    spec = forward(torch, eng, x)
    F = spec.shape[0]
    N = (F - 1) * r.H + r.W
    full = eng.istft_batch(spec)
    # n_out at and past the end; a NULL n_out; n_frames = 0
    got = C.c_size_t(99)
    out = torch.empty((N, 2), device="cuda")
    sp = C.c_void_p(spec.data_ptr())
    assert eng._lib.sgx_istft_batch(eng._ctx, sp, F, N - 5, 100, C.c_void_p(out.data_ptr()), C.byref(got)) == _lib.SGX_OK
    assert got.value == 5
    assert eng._lib.sgx_istft_batch(eng._ctx, sp, F, N, 100, C.c_void_p(out.data_ptr()), C.byref(got)) == _lib.SGX_OK
    assert got.value == 0
    assert eng._lib.sgx_istft_batch(eng._ctx, sp, F, 0, N, C.c_void_p(out.data_ptr()), None) == _lib.SGX_OK
    assert eng._lib.sgx_istft_batch(eng._ctx, C.c_void_p(0), 0, 0, N, C.c_void_p(0), C.byref(got)) == _lib.SGX_OK
    assert got.value == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), full.view(torch.int32))
    assert eng.istft_batch(spec[:0]).shape == (0, 2)
    # null buffers where samples exist
    assert eng._lib.sgx_istft_batch(eng._ctx, C.c_void_p(0), F, 0, N, C.c_void_p(out.data_ptr()), C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert eng._lib.sgx_istft_batch(eng._ctx, sp, F, 0, N, C.c_void_p(0), C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert got.value == 0
    # a context only kernel 11 serves
    big = engine(es.ROUTE["large_w6001_chirp_lr"])
    assert big.istft_supported() == 0
    rc = big._lib.sgx_istft_batch(big._ctx, sp, 1, 0, 10, C.c_void_p(out.data_ptr()), C.byref(got))
    assert rc == _lib.SGX_ERR_UNSUPPORTED and got.value == 0
    # a non-default stream: the call only enqueues (the tables were built by the calls above), and gives the same bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(400_000_000)
        other = eng.istft_batch(spec)
        pending = not side.query()
    side.synchronize()
    assert pending, "the host must have run ahead of the stream"
    assert torch.equal(other.view(torch.int32), full.view(torch.int32))
