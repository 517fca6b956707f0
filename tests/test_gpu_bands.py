"""sgx_bands_batch: PCM to the magnitude_in means of the context's log-frequency rows (include/sgx.h), all through the C ABI.

The contract is bit-identity with the two-call composition sgx_stft_batch -> sgx_magnitude_in over the ranges
(edge[py], edge[py + 1]) of sgx_bin_edges: both build their tables with the same host code and the library rounds every float
operation once, so any difference is a bug.  Checked on the fused kernels (K1, real-input K1R, the mixed-radix plans) and on the
two-kernel route, against the CPU oracle on sampled frames, fused against split, across palettes, on sub-ranges, through the live
ring, on a non-default stream, and at config 3's full size."""
import ctypes as C

import numpy as np
import pytest

import oracle
from spectrogram_rs_amd import SpectrogramEngine, _lib

pytestmark = pytest.mark.gpu

SR = 48000.0
FRAMES = 80
INTERPS = {"cubic": _lib.INTERP_CUBIC, "cosine": _lib.INTERP_COSINE}

# name: (engine keyword arguments, expected sgx_bands_fused)
CASES = {
    "w2048_h256_mono": (dict(window_samples=2048, hop_samples=256), 1),
    "w2048_h256_lr": (dict(window_samples=2048, hop_samples=256, channels=2), 1),
    "w2048_h256_paired": (dict(window_samples=2048, hop_samples=256, paired_frames=True), 1),
    "w2048_h256_complex": (dict(window_samples=2048, hop_samples=256, complex_mono=True), 1),
    "w2048_h200_mono": (dict(window_samples=2048, hop_samples=200), 1),
    "w2048_h200_lr": (dict(window_samples=2048, hop_samples=200, channels=2), 1),
    "w2048_h200_paired": (dict(window_samples=2048, hop_samples=200, paired_frames=True), 1),
    "w2048_h200_complex": (dict(window_samples=2048, hop_samples=200, complex_mono=True), 1),
    "w2048_ch4": (dict(window_samples=2048, hop_samples=256, channels=4), 1),
    "w2048_ch8": (dict(window_samples=2048, hop_samples=256, channels=8), 1),
    "w2400_h93_mono": (dict(window_samples=2400, hop_samples=93), 1),
    # (l, r) at W 2400: rows from the tuned 4800-point kernel, which no fused column reproduces bit for bit: the two-kernel route
    "w2400_h93_lr": (dict(window_samples=2400, hop_samples=93, channels=2), 0),
    "w2400_h93_ch4": (dict(window_samples=2400, hop_samples=93, channels=4), 1),
    "w2205_mono": (dict(window_samples=2205, hop_samples=551), 1),
    "w1102_chirpz": (dict(window_samples=1102, hop_samples=275), 0),
    "w8192_h512": (dict(window_samples=8192, hop_samples=512), 0),
    "w19200_large": (dict(window_samples=19200, hop_samples=4800, large_transforms=True), 0),
    "r256": (dict(window_samples=2048, hop_samples=256, rows=256), 1),
    "r1024": (dict(window_samples=2048, hop_samples=256, rows=1024), 1),
    "r2048": (dict(window_samples=2048, hop_samples=256, rows=2048), 0),
    "fmin_fmax": (dict(window_samples=2048, hop_samples=256, f_min=100.0, f_max=8000.0), 1),
}


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def make(name, interp, **extra):
    kw, _ = CASES[name]
    return SpectrogramEngine(SR, device=0, interp=INTERPS[interp], **kw, **extra)


def two_call(eng, pcm):
    """sgx_stft_batch, then sgx_magnitude_in over the ranges of sgx_bin_edges: [frames][pairs][R][2]"""
    mags = eng.stft_batch(pcm)
    edges = eng.bin_edges()
    ranges = np.stack([edges[:-1], edges[1:]], 1)
    out = eng.magnitude_in(mags.reshape(-1, eng.M, 2), ranges)
    return mags, out.reshape(mags.shape[0], eng.pairs, eng.R, 2)


@pytest.mark.parametrize("interp", sorted(INTERPS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_composition_oracle_and_split(name, interp):
    import torch

    eng = make(name, interp)
    n_samples = eng.W + (FRAMES - 1) * eng.H
    pcm = eng.white_noise(n_samples, seed=0x5EED0101)
    bands = eng.bands_batch(pcm)
    mags, ref = two_call(eng, pcm)
    torch.cuda.synchronize()
    assert bands.shape == (FRAMES, eng.pairs, eng.R, 2)
    # 1. the two-call composition, bit for bit
    assert np.array_equal(bits(bands), bits(ref)), f"{name}/{interp}: bands differ from stft_batch + magnitude_in"
    # 2. the CPU oracle over the engine's own rows on sampled frames (first and last pair)
    got, own = bands.cpu().numpy(), mags.cpu().numpy()
    edges = eng.bin_edges()
    rng = np.random.default_rng(7)
    frames = sorted(set([0, FRAMES - 1] + list(rng.choice(FRAMES, 64, replace=False))))
    for f in frames:
        for pair in sorted({0, eng.pairs - 1}):
            want = np.stack([oracle.magnitude_in(own[f, pair], eng.info.sample_rate_u32, float(edges[py]), float(edges[py + 1]),
                                                 INTERPS[interp]) for py in range(eng.R)])
            assert np.array_equal(got[f, pair].view(np.uint32), want.view(np.uint32)), f"{name}/{interp}: frame {f} pair {pair}"
    # 3. fused against split, and where the fused kernel must run
    assert eng.bands_fused == CASES[name][1], f"{name}: bands_fused"
    if not (eng.info.stft_kernel == 9 and eng.channels <= 2):
        assert eng.bands_fused >= (eng.info.render_path & 1), f"{name}: render_batch fuses here, bands_batch must too"
    split = make(name, interp, fused_render=False)
    assert split.bands_fused == 0
    other = split.bands_batch(pcm)
    torch.cuda.synchronize()
    assert np.array_equal(bits(bands), bits(other)), f"{name}/{interp}: fused and split differ"


@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr", "w2400_h93_mono", "w2400_h93_ch4", "w2205_mono"])
def test_palette_does_not_matter(name):
    import torch

    eng = make(name, "cubic")
    pcm = eng.white_noise(eng.W + (FRAMES - 1) * eng.H, seed=3)
    fused = eng.bands_fused
    base = bits(eng.bands_batch(pcm))
    eng.set_builtin_scheme("red_blue", stereo=True)
    assert eng.bands_fused == fused
    assert np.array_equal(bits(eng.bands_batch(pcm)), base)
    ramp = np.array([[0, 0, 0], [40, 0, 80], [120, 0, 120], [200, 40, 60], [250, 120, 0], [255, 220, 60], [255, 255, 255]], np.uint8)
    eng.set_gradient(ramp)
    assert eng.bands_fused == fused
    assert np.array_equal(bits(eng.bands_batch(pcm)), base)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_paired", "w2048_h200_lr", "w2400_h93_mono", "w8192_h512"])
def test_slicing_and_arguments(name):
    import torch

    eng = make(name, "cubic")
    pcm = eng.white_noise(eng.W + (FRAMES - 1) * eng.H, seed=11)
    full = eng.bands_batch(pcm)
    for first, count in [(0, 1), (1, 7), (13, 30), (FRAMES - 5, None), (FRAMES - 1, 100)]:
        part = eng.bands_batch(pcm, first_frame=first, max_frames=count)
        end = FRAMES if count is None else min(first + count, FRAMES)
        assert np.array_equal(bits(part), bits(full[first:end])), f"{name}: [{first}, {end})"
    torch.cuda.synchronize()
    lib, got = eng._lib, C.c_size_t(123)
    out = torch.empty(4, dtype=torch.float32, device=eng.device)
    short = pcm[:(eng.W - 1) * eng.channels]
    assert lib.sgx_bands_batch(eng._ctx, C.c_void_p(short.data_ptr()), eng.W - 1, 0, 10, C.c_void_p(out.data_ptr()), C.byref(got)) == 0
    assert got.value == 0
    n = pcm.numel() // eng.channels
    assert lib.sgx_bands_batch(eng._ctx, None, n, 0, 10, C.c_void_p(out.data_ptr()), C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_bands_batch(eng._ctx, C.c_void_p(pcm.data_ptr()), n, 0, 10, None, C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_bands_batch(None, C.c_void_p(pcm.data_ptr()), n, 0, 10, C.c_void_p(out.data_ptr()), C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_bands_fused(None) == _lib.SGX_ERR_INVALID_ARG


@pytest.mark.parametrize("W,H", [(2048, 256), (2400, 93)])
def test_live_tick_bands(W, H):
    import torch

    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=H, channels=2, device=0)
    ring = eng.live(16384)
    pcm = eng.white_noise(W + 40 * H, seed=5)
    host = pcm.cpu().numpy()
    assert ring.push(host, 2) == host.size // 2
    got = ring.tick("bands")
    want = eng.bands_batch(pcm)
    torch.cuda.synchronize()
    assert got.shape == (41, eng.R, 2)
    assert np.array_equal(got.view(np.uint32), want.reshape(41, eng.R, 2).cpu().numpy().view(np.uint32))
    ring.close()


def test_stream_ordered_and_asynchronous():
    """queued behind a long kernel on a non-default stream, the call returns before that kernel ends; the input is written on the
    same stream behind the sleep, so work put anywhere else would read NaN"""
    import torch

    for name in ["w2048_h256_mono", "w2400_h93_ch4", "w8192_h512"]:
        eng = make(name, "cubic")
        n = eng.W + (FRAMES - 1) * eng.H
        ref = eng.bands_batch(eng.white_noise(n, seed=21))
        torch.cuda.synchronize()
        pcm = torch.full((n * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
        out = torch.full((FRAMES, eng.pairs, eng.R, 2), -1.0, dtype=torch.float32, device=eng.device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        eng.set_stream(s.cuda_stream)
        lib, got = eng._lib, C.c_size_t(0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(400_000_000)
        eng._check(lib.sgx_synth_white_noise(eng._ctx, C.c_void_p(pcm.data_ptr()), 0, n, eng.channels, 21))
        eng._check(lib.sgx_bands_batch(eng._ctx, C.c_void_p(pcm.data_ptr()), n, 0, FRAMES, C.c_void_p(out.data_ptr()), C.byref(got)))
        done = torch.cuda.Event()
        done.record(s)
        assert not done.query(), f"{name}: sgx_bands_batch waited for the stream"
        eng.sync()
        assert got.value == FRAMES
        assert np.array_equal(bits(out), bits(ref)), name
        eng.set_stream(0)


@pytest.mark.parametrize("interp", sorted(INTERPS))
def test_full_size_config3(interp):
    """config 3's stream: 1e6 mono frames at W 2048 / H 256 (8.2 GB of bands); 1 024 sampled columns against magnitude_in over the
    engine's own rows of those frames"""
    import torch

    frames, W, H = 1_000_000, 2048, 256
    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=H, device=0, interp=INTERPS[interp])
    assert eng.bands_fused == 1
    pcm = eng.white_noise(W + (frames - 1) * H, seed=0x5EED0001)
    bands = eng.bands_batch(pcm)
    edges = eng.bin_edges()
    ranges = np.stack([edges[:-1], edges[1:]], 1)
    rng = np.random.default_rng(1)
    picks = np.unique(np.concatenate([[0, frames - 1], rng.choice(frames, 1022, replace=False)]))
    mags = torch.empty((1, 1, eng.M, 2), dtype=torch.float32, device=eng.device)
    want = torch.empty((len(picks), eng.R, 2), dtype=torch.float32, device=eng.device)
    for i, f in enumerate(picks):
        eng.stft_batch(pcm, first_frame=int(f), max_frames=1, out=mags)
        eng.magnitude_in(mags.reshape(-1, eng.M, 2), ranges, out=want[i:i + 1])
    got = bands[torch.as_tensor(picks, device=eng.device), 0]
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(want))
    del bands, pcm
    torch.cuda.empty_cache()
