"""sgx_stft_batch_complex: the complex (L, R) spectra of the split on every transform route (tests/edge_signals.py: the route table and
the edge streams), against the complex float64 truth -- the numpy DFT of Hann * l and Hann * r, times 2 / W.  Each row first asserts the
kernel and render_path bits it names.  Then: every frame of its edge stream and of seeded white noise against the truth (silent frames
exactly zero); |L|, |R| against the same context's sgx_stft_batch within a few float32 ulps; single impulses in one channel against
x0 w[n0] e^{-2 pi i k n0 / 2W} 2 / W (the rotation of the right channel and the L / R order); sub-ranges bit-identical to the full run
(kernel 11's chunk boundaries included); rows past byte 2^32; the call's contract.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import edge_signals as es
import oracle
from conftest import REL_TOL, chirpz_bound

pytestmark = pytest.mark.gpu

ROWS = [r.name for r in es.ROUTES]
_cache = {}

# Multiples of the row's floor every frame is held to, per complex bin: |dC| <= REL_TOL max(|C|, floor peak).  The magnitude floors were
# measured on |C| only; a complex value also carries the tangential (phase) part of the rounding error, which a magnitude never sees.
# The edge streams keep test_gpu_edges.EDGE_BOUND's measured flat-spectrum exception (2.5 x, an independent float32 FFT reads up to
# 3.8 x on them); white noise is held to the row's own bound.
COMPLEX_BOUND = {"noise": 1.0, "flat spectra": 2.5}
FLAT_SPECTRUM_ROWS = {
    "k1_lr_h256", "k1_lr_h58", "k1_paired_mono", "k1_ch8", "k16_lr_h512", "k16_lr_h300", "k16_ch8_h512", "k16_ch8_h300",
    "k16_mono_h512", "k48_lr", "k48_paired_mono", "mixed_w2400_generic", "mixed_w2400_ch4", "mixed_w4096_lr", "mixed_w735_runtime_lr",
    "chirpz_w1102_lr", "chirpz_w1852_lr", "bluestein_w1102", "generic_w2048_lr", "large_w19200_lr", "large_w6001_chirp_lr",
    "large_w65537_chirp_lr", "large_w6001_chunks"}
# Rows outside that exception whose edge stream reads above 1 x once the phase counts, measured on the MI355X (worst frame, complex
# against the complex truth): K1 (s, s) 1.30, K1R H 100 1.13, generic W 2048 mono 1.10, kernel 11 W 10290 mono 1.08, chirp-z real-input
# W 1102 1.05, mixed radix W 1024 (l, r) 1.01.  Their magnitudes hold 1 x (tests/test_gpu_edges.py); white noise holds 1 x on every row.
PHASE_EDGE_BOUND = 1.5
PHASE_EDGE_ROWS = {"k1_complex_mono", "k1r_h100", "generic_w2048_mono", "large_w10290_mono", "chirpz_w1102_real", "mixed_w1024_lr"}
# |L|, |R| in float64 against sgx_stft_batch's float32 value: the square root (1 ulp), the sum of squares and, where the scale is applied
# after the root (not a power of two riding on the window), one multiply per component
HYPOT_ULPS = 4.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def engine(r, **extra):
    from spectrogram_rs_amd import SpectrogramEngine
    return SpectrogramEngine(es.SR, device=0, **r.engine_kwargs(), **extra)


def to_dev(torch, r, pcm):
    flat = torch.from_numpy(np.ascontiguousarray(pcm, np.float32).reshape(-1)).cuda()
    if not r.align4:
        return flat
    buf = torch.zeros(flat.numel() + 1, dtype=torch.float32, device="cuda")
    buf[1:] = flat
    dev = buf[1:]
    assert dev.data_ptr() % 8 == 4
    return dev


def truth_complex(lr, W):
    """[W - 1][2] complex128: (L, R) = (DFT(Hann * l), DFT(Hann * r)) * 2 / W at k = 1 .. W - 1 (float32 window products, as the kernels)"""
    win = es.hann(W)
    lr = np.ascontiguousarray(lr, np.float32).reshape(-1, 2)[:W]
    z = np.stack([lr[:, 0] * win, lr[:, 1] * win], 0).astype(np.float64)
    F = np.fft.fft(z, n=2 * W, axis=1)[:, 1:W] * (2.0 / W)
    return F.T


def complex_error(x, ref, floor, peak):
    """worst |x - ref| / (REL_TOL max(|ref|, floor peak)) over the complex values of one frame"""
    allow = np.maximum(REL_TOL * np.maximum(np.abs(ref), floor * peak), 1e-30)
    return float((np.abs(np.asarray(x, np.complex128) - ref) / allow).max())


def noise_stream(r, frames=24, seed=11):
    n = (frames - 1) * r.H + r.W
    return (oracle.white_noise(n * r.channels, seed=seed + r.W + r.channels) * np.float32(0.25)).reshape(n, r.channels)


def case(torch, name):
    """(route, edge stream, engine, device stream, complex rows, magnitude rows), built once per row"""
    if name not in _cache:
        r = es.ROUTE[name]
        s = es.build_stream(r)
        eng = engine(r)
        dev = to_dev(torch, r, s.pcm)
        cx = eng.stft_batch_complex(dev).cpu().numpy()
        mags = eng.stft_batch(dev).cpu().numpy()
        _cache[name] = (r, s, eng, dev, cx, mags)
    return _cache[name]


def hold_to_truth(name, r, frames, frame_of, got, bound):
    """every frame of `got` ([F][pairs][M][2] complex64) against the truth; silent transforms exactly zero.  Returns (worst, silent)"""
    W = r.W
    truths = {}

    def truth(t, p):
        if (t, p) not in truths:
            truths[(t, p)] = truth_complex(es.frame_lr(frame_of(t), p), W)
        return truths[(t, p)]

    worst, where, silent_frames = 0.0, None, 0
    for t in range(frames):
        silent = es.windowed_silent(frame_of(t), W)
        for p in range(r.pairs):
            ref = truth(t, p)
            quiet = bool(silent[2 * p:2 * p + 2].all()) if r.channels > 1 else bool(silent[0])
            peak = float(np.abs(ref).max())
            if r.paired:
                q = t ^ 1
                partner = float(np.abs(truth(q, 0)).max()) if q < frames else 0.0
                if quiet and partner == 0.0:
                    assert not got[t, p].any(), (name, t, "a silent transform must be exactly zero")
                    silent_frames += 1
                    continue
                peak = max(peak, partner)
            elif quiet:
                assert not got[t, p].any(), (name, t, p, "a silent frame must be exactly zero")
                silent_frames += 1
                continue
            err = complex_error(got[t, p], ref, r.floor, peak)
            if err > worst:
                worst, where = err, (t, p)
    print(f"COMPLEX-RATIO {name} worst {worst:.4f} at {where} (bound {bound})")
    assert worst <= bound, (name, where, worst, bound)
    return worst, where, silent_frames


def edge_bound(r):
    if r.name in FLAT_SPECTRUM_ROWS:
        return COMPLEX_BOUND["flat spectra"]
    own = chirpz_bound(r.W) if r.kernel == 4 else COMPLEX_BOUND["noise"]
    return max(own, PHASE_EDGE_BOUND) if r.name in PHASE_EDGE_ROWS else own


def noise_bound(r):
    return chirpz_bound(r.W) if r.kernel == 4 else COMPLEX_BOUND["noise"]


@pytest.mark.parametrize("name", ROWS)
def test_route(torch_cuda, name):
    r, _, eng, _, cx, _ = case(torch_cuda, name)
    info = eng.info
    assert info.stft_kernel == r.kernel, (name, info.stft_kernel)
    assert info.render_path & r.bits_set == r.bits_set and info.render_path & r.bits_clear == 0, (name, info.render_path)
    assert cx.dtype == np.complex64 and cx.shape == (cx.shape[0], r.pairs, r.W - 1, 2)


@pytest.mark.parametrize("name", ROWS)
def test_edge_stream_against_the_truth(torch_cuda, name):
    r, s, _, _, cx, _ = case(torch_cuda, name)
    assert cx.shape[0] == s.frames
    worst, where, silent = hold_to_truth(name, r, s.frames, s.frame, cx, edge_bound(r))
    assert silent >= 1
    print(f"COMPLEX-EDGE-RATIO {name} worst {worst:.4f} at {where} (bound {edge_bound(r)}), {silent} silent exactly zero")


@pytest.mark.parametrize("name", ROWS)
def test_white_noise_against_the_truth(torch_cuda, name):
    torch = torch_cuda
    r = es.ROUTE[name]
    frames = 24 if r.W < 1 << 16 else 4
    pcm = noise_stream(r, frames)
    eng = case(torch, name)[2]
    got = eng.stft_batch_complex(to_dev(torch, r, pcm)).cpu().numpy()
    H, W = r.H, r.W
    worst, where, _ = hold_to_truth(name, r, frames, lambda t: pcm[t * H:t * H + W], got, noise_bound(r))
    print(f"COMPLEX-NOISE-RATIO {name} worst {worst:.4f} at {where} (bound {noise_bound(r)})")


@pytest.mark.parametrize("name", ROWS)
def test_magnitudes_are_the_complex_moduli(torch_cuda, name):
    r, s, _, _, cx, mags = case(torch_cuda, name)
    h = np.abs(cx.astype(np.complex128))
    m = mags.astype(np.float64)
    assert not np.isnan(m).any() and not np.isnan(h).any()
    # (components below 2^-63 have float32 squares below the normal range, and sgx_stft_batch's magnitude of such a bin flushes to 0
    # -- measured on K16's edge streams: |L| about 2^-63 where the magnitude is 0.  The ulp is taken at 2^-40 or above.)
    ulp = np.spacing(np.maximum(m, 2.0 ** -40).astype(np.float32)).astype(np.float64)
    ratio = float((np.abs(h - m) / ulp).max())
    print(f"COMPLEX-HYPOT-ULPS {name} worst {ratio:.3f} (bound {HYPOT_ULPS})")
    assert ratio <= HYPOT_ULPS, (name, ratio)


# an impulse in ONE channel: the driven half is x0 w[n0] e^{-2 pi i k n0 / 2W} 2 / W, the other half zero.  A right channel stored as the
# unrotated difference, or L and R swapped, misses by about the peak (1 / REL_TOL allowances).
IMPULSE_ROWS = ["k1_lr_h256", "k1_ch4", "k16_lr_h512", "k16_ch8_h512", "k48_lr", "mixed_w2400_generic", "mixed_w735_runtime_lr",
                "chirpz_w1852_lr", "bluestein_w1102", "generic_w256_lr", "large_w19200_lr", "large_w6001_chirp_lr"]


def impulse_truth(W, n0, x0):
    k = np.arange(1, W)
    return x0 * float(es.hann(W)[n0]) * np.exp(-2j * np.pi * k * n0 / (2 * W)) * (2.0 / W)


@pytest.mark.parametrize("name", IMPULSE_ROWS)
@pytest.mark.parametrize("side", [0, 1])
def test_impulse_phase_and_channel_order(torch_cuda, name, side):
    torch = torch_cuda
    r = es.ROUTE[name]
    W, C = r.W, r.channels
    eng = case(torch, name)[2]
    for n0, x0 in ((W // 3 + 5, 1.0), (W // 2, -0.75), (7, 0.5)):
        pcm = np.zeros((W, C), np.float32)
        pair = r.pairs - 1
        pcm[n0, 2 * pair + side] = x0
        got = eng.stft_batch_complex(to_dev(torch, r, pcm)).cpu().numpy().astype(np.complex128)
        assert got.shape == (1, r.pairs, W - 1, 2)
        ref = impulse_truth(W, n0, x0)
        allow = REL_TOL * np.abs(ref)
        worst_d = float((np.abs(got[0, pair, :, side] - ref) / allow).max())
        worst_o = float((np.abs(got[0, pair, :, 1 - side]) / allow).max())
        print(f"COMPLEX-IMPULSE {name} side {side} n0 {n0}: driven {worst_d:.4f}, other {worst_o:.4f}")
        assert worst_d <= 1.0 and worst_o <= 1.0, (name, side, n0, worst_d, worst_o)
        for p in range(r.pairs - 1):   # the other pairs are silent
            assert not got[0, p].any()


@pytest.mark.parametrize("name", ["k1r_h256", "k1r_h100", "mixed_w2400_real", "chirpz_w1102_real", "large_w10290_mono"])
def test_mono_impulse_both_halves(torch_cuda, name):
    torch = torch_cuda
    r = es.ROUTE[name]
    W = r.W
    eng = case(torch, name)[2]
    for n0, x0 in ((W // 3 + 5, 1.0), (W // 2 + 1, -0.5)):
        pcm = np.zeros((W, 1), np.float32)
        pcm[n0, 0] = x0
        got = eng.stft_batch_complex(to_dev(torch, r, pcm)).cpu().numpy().astype(np.complex128)
        ref = impulse_truth(W, n0, x0)
        for half in (0, 1):
            worst = float((np.abs(got[0, 0, :, half] - ref) / (REL_TOL * np.abs(ref))).max())
            print(f"COMPLEX-MONO-IMPULSE {name} n0 {n0} half {half}: {worst:.4f}")
            assert worst <= 1.0, (name, n0, half, worst)


@pytest.mark.parametrize("name", ROWS)
def test_sub_ranges_are_bit_identical(torch_cuda, name):
    r, s, eng, dev, cx, _ = case(torch_cuda, name)
    tf = [sl.frame for sl in s.target_slots()]
    even = next(t for t in tf[1:] if t % 2 == 0)
    odd = next((t for t in tf if t % 2 == 1), None)
    calls = [(even, 1), (even, 3), (tf[-1], 1)]
    if odd is not None:
        calls += [(odd, 1), (odd, 4), (odd, None)]
    if r.chunk_targets:
        for b in es.chunk_boundary_frames(r.W, r.pairs, s.frames):
            calls += [(max(b - 1, 0), 2), (b, None)]
    for first, count in calls:
        part = eng.stft_batch_complex(dev, first_frame=first, max_frames=count).cpu().numpy()
        end = s.frames if count is None else min(s.frames, first + count)
        assert np.array_equal(part.view(np.uint32), cx[first:end].view(np.uint32)), (name, first, count)


def test_rows_past_4_gib(torch_cuda):
    torch = torch_cuda
    r = es.ROUTE["k1_lr_h256"]
    W, H = r.W, r.H
    row_bytes = (W - 1) * 16
    frames = 140_000
    assert frames * row_bytes > 2 ** 32 + 8 * row_bytes
    n = (frames - 1) * H + W
    eng = engine(r)
    dev = eng.white_noise(n, seed=3)
    full = eng.stft_batch_complex(dev)
    t0 = 2 ** 32 // row_bytes        # the row holding byte 2^32
    for t in (t0 - 1, t0, t0 + 1, frames - 1):
        part = eng.stft_batch_complex(dev, first_frame=t, max_frames=2)
        assert torch.equal(torch.view_as_real(part).view(torch.int32),
                           torch.view_as_real(full[t:t + part.shape[0]]).view(torch.int32)), t
        frame = dev[2 * t * H:2 * (t * H + W)].cpu().numpy().reshape(W, 2)
        ref = truth_complex(frame, W)
        got = full[t, 0].cpu().numpy()
        err = complex_error(got, ref, r.floor, float(np.abs(ref).max()))
        print(f"COMPLEX-4GIB frame {t}: {err:.4f}")
        assert err <= COMPLEX_BOUND["noise"], (t, err)
    del full, dev
    torch.cuda.empty_cache()


def test_contract(torch_cuda):
    torch = torch_cuda
    from spectrogram_rs_amd import _lib
    r = es.ROUTE["k1_lr_h256"]
    eng = case(torch, r.name)[2]
    # too few samples: nothing produced, not an error
    short = torch.zeros((r.W - 1) * 2, device="cuda")
    assert eng.stft_batch_complex(short).shape == (0, 1, r.W - 1, 2)
    got = C.c_size_t(99)
    rc = eng._lib.sgx_stft_batch_complex(eng._ctx, C.c_void_p(short.data_ptr()), r.W - 1, 0, 4, C.c_void_p(0), C.byref(got))
    assert rc == _lib.SGX_OK and got.value == 0
    # a null buffer where frames exist
    pcm = torch.from_numpy(noise_stream(r, 4).reshape(-1)).cuda()
    rc = eng._lib.sgx_stft_batch_complex(eng._ctx, C.c_void_p(pcm.data_ptr()), pcm.numel() // 2, 0, 4, C.c_void_p(0), C.byref(got))
    assert rc == _lib.SGX_ERR_INVALID_ARG and got.value == 0
    # a non-default stream: the same bytes
    ref = eng.stft_batch_complex(pcm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = eng.stft_batch_complex(pcm)
    side.synchronize()
    assert torch.equal(torch.view_as_real(other).view(torch.int32), torch.view_as_real(ref).view(torch.int32))
    # the float32 out= and the complex64 out= hold the same bytes; the result views the caller's buffer
    f32 = torch.empty(ref.shape + (2,), dtype=torch.float32, device="cuda")
    c64 = torch.empty(ref.shape, dtype=torch.complex64, device="cuda")
    a = eng.stft_batch_complex(pcm, out=f32)
    b = eng.stft_batch_complex(pcm, out=c64)
    assert a.data_ptr() == f32.data_ptr() and b.data_ptr() == c64.data_ptr()
    assert torch.equal(f32.view(torch.int32), torch.view_as_real(c64).view(torch.int32))
    assert torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(ref).view(torch.int32))


# real-input mode and frame pairs store X itself in both halves (the (s, s) dataflow of the other mono contexts computes the halves as two
# float32 evaluations of X: held to the truth above, not to each other)
@pytest.mark.parametrize("name", ["k1r_h256", "k1r_h100", "k1r_h256_align4", "k1_paired_mono", "k48_paired_mono", "mixed_w2205_real",
                                  "mixed_w2400_real", "mixed_w1024_real", "mixed_w5000_runtime_real", "chirpz_w1102_real"])
def test_mono_halves_are_identical(torch_cuda, name):
    r, s, _, _, cx, _ = case(torch_cuda, name)
    assert r.channels == 1
    v = cx.view(np.uint32).reshape(cx.shape[0], 1, r.W - 1, 2, 2)
    assert np.array_equal(v[:, :, :, 0], v[:, :, :, 1]), name


# the rows that once came out different from run to run (a 16-byte store whose data register was overwritten one wait state after it):
# repeated calls on one stream must give the same bytes, and those of the cached first run
@pytest.mark.parametrize("name", ["k48_lr", "k48_paired_mono", "k16_lr_h512", "k16_ch8_h512", "k16_mono_h512", "k16_lr_h300",
                                  "k1_lr_h256", "k1_paired_mono", "k1r_h256", "k1r_h100"])
def test_repeated_runs_are_bit_identical(torch_cuda, name):
    torch = torch_cuda
    r, s, eng, dev, cx, _ = case(torch, name)
    first = torch.from_numpy(cx.view(np.int32)).cuda()
    for _ in range(8):
        again = torch.view_as_real(eng.stft_batch_complex(dev)).view(torch.int32)
        assert torch.equal(again.reshape(first.shape), first), name
