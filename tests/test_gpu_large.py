"""The multi-pass transform (SGX_FLAG_LARGE_TRANSFORM, stft_kernel 11, csrc/stft_large.hip): lengths no in-LDS kernel serves, W up to
2^20, against the float64 truth of the reference's frame (oracle.np_truth_frame) -- the float32 oracle's prime sums are far too slow
at these lengths.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import oracle
from conftest import FLOOR_WIDE, mags_error

pytestmark = pytest.mark.gpu

SR = 48000.0
# Multiples of the FLOOR_WIDE bound this path is held to (in the manner of conftest.KERNEL_BOUND): 1 x everywhere.  Measured worst ratio
# (profiles/r07_large.txt): 0.46 .. 0.64 for the direct lengths up to 2^21 points, 0.66 .. 0.78 for chirp-z (6001 stereo the worst).
LARGE_BOUND = {"default": 1.0}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def engine(W, H, channels=2, large=True, sr=SR, **kw):
    from spectrogram_rs_amd import SpectrogramEngine
    return SpectrogramEngine(sr, window_samples=W, hop_samples=H, channels=channels, device=0, large_transforms=large, **kw)


def noise(n_samples, channels, seed):
    return oracle.white_noise(n_samples * channels, seed=seed).reshape(n_samples, channels)


def truth(pcm, W, H, frames, pair=0):
    """[frames][M][2] float64 truth of pair `pair` (mono: (s, s))"""
    out = []
    for t in range(frames):
        x = pcm[t * H:t * H + W]
        lr = np.stack([x[:, 0], x[:, 0]], 1) if x.shape[1] == 1 else x[:, 2 * pair:2 * pair + 2]
        out.append(oracle.np_truth_frame(lr, W))
    return np.stack(out)


def check_against_truth(got, pcm, W, H, pairs=1, bound=LARGE_BOUND["default"]):
    for p in range(pairs):
        ref = truth(pcm, W, H, got.shape[0], p)
        for t in range(got.shape[0]):   # every frame on its own
            err = mags_error(got[t, p], ref[t], floor=FLOOR_WIDE)
            assert err <= bound, (W, H, p, t, err)


def run(torch, eng, pcm, **kw):
    return eng.stft_batch(torch.from_numpy(np.ascontiguousarray(pcm)).cuda().reshape(-1), **kw).cpu().numpy()


def test_app_window_at_384k(torch_cuda):
    # the application's 0.05 s at a 384 kHz capture: 2W = 38400 = 2^9 3 5^2, refused without the flag
    from spectrogram_rs_amd import SpectrogramEngine
    eng = SpectrogramEngine(384000.0, period=0.05, stride=0.0125, channels=2, device=0, large_transforms=True)
    assert eng.W == 19200 and eng.H == 4800 and eng.info.stft_kernel == 11 and eng.info.render_path == 0
    pcm = noise(19200 + 39 * 4800, 2, seed=384)
    got = run(torch_cuda, eng, pcm)
    assert got.shape == (40, 1, 19199, 2)
    check_against_truth(got, pcm, 19200, 4800)


@pytest.mark.parametrize("W,frames", [
    (16384, 6),       # 2W = 32768: the usual high-resolution window
    (17640, 6),       # 0.05 s at 352.8 kHz: 35280 = 2^4 3^2 5 7^2
    (48000, 4),       # 1 s at 48 kHz: 96000
    (10290, 6),       # 20580 = 2^2 3 5 7^3: smooth, just past the LDS
    (6001, 6),        # 12002 = 2 17 353: chirp-z
    (65537, 3),       # prime W: chirp-z
    (1 << 20, 2),     # the longest: 2W = 2^21
])
def test_lengths_beyond_the_lds(torch_cuda, W, frames):
    H = W // 2 + 3
    eng = engine(W, H)
    assert eng.info.stft_kernel == 11 and eng.P == 2 * W
    pcm = noise(W + (frames - 1) * H, 2, seed=W)
    got = run(torch_cuda, eng, pcm)
    assert got.shape == (frames, 1, W - 1, 2)
    check_against_truth(got, pcm, W, H)


def test_flag_changes_nothing_where_an_in_lds_kernel_serves(torch_cuda):
    for W, kernel in ((2400, 9), (10240, 6), (8192, 10), (5003, 4)):
        with_flag, without = engine(W, 301), engine(W, 301, large=False)
        assert with_flag.info.stft_kernel == kernel == without.info.stft_kernel, W
        assert with_flag.info.render_path == without.info.render_path, W
        pcm = noise(W + 5 * 301, 2, seed=W)
        assert np.array_equal(run(torch_cuda, with_flag, pcm), run(torch_cuda, without, pcm)), W


def test_refusals_name_the_length_and_the_flag(torch_cuda):
    from spectrogram_rs_amd import SgxError
    with pytest.raises(SgxError) as ei:
        engine((1 << 20) + 1, 4096)
    assert ei.value.code == -2 and str(2 * ((1 << 20) + 1)) in str(ei.value)
    with pytest.raises(SgxError) as ei:
        engine(16384, 4096, large=False)
    assert ei.value.code == -2 and "32768" in str(ei.value) and "SGX_FLAG_LARGE_TRANSFORM" in str(ei.value)


@pytest.mark.parametrize("W", [6001, 16384])
@pytest.mark.parametrize("channels", [1, 2, 4])
def test_channels(torch_cuda, W, channels):
    H = W // 4
    eng = engine(W, H, channels=channels)
    assert eng.info.stft_kernel == 11
    pcm = noise(W + 4 * H, channels, seed=channels)
    got = run(torch_cuda, eng, pcm)
    assert got.shape == (5, max(1, channels // 2), W - 1, 2)
    check_against_truth(got, pcm, W, H, pairs=max(1, channels // 2))


@pytest.mark.parametrize("W", [6001, 16384])
@pytest.mark.parametrize("hop", [1, "quarter", "long"])
def test_hops(torch_cuda, W, hop):
    H = {1: 1, "quarter": W // 4, "long": W + 777}[hop]
    eng = engine(W, H)
    pcm = noise(W + 6 * H + H // 2, 2, seed=H)
    got = run(torch_cuda, eng, pcm)
    assert got.shape[0] == 7
    check_against_truth(got, pcm, W, H)


def test_short_stream_and_sub_ranges(torch_cuda):
    torch = torch_cuda
    W, H = 6001, 1000
    eng = engine(W, H)
    assert run(torch, eng, noise(W - 1, 2, seed=1)).shape == (0, 1, W - 1, 2)
    pcm = noise(W + 11 * H, 2, seed=2)
    full = run(torch, eng, pcm)
    assert full.shape[0] == 12
    for first, count in ((0, 1), (3, 4), (11, 5), (5, None)):
        part = run(torch, eng, pcm, first_frame=first, max_frames=count)
        end = 12 if count is None else min(12, first + count)
        assert np.array_equal(part, full[first:end]), (first, count)
    assert run(torch, eng, pcm, first_frame=12).shape[0] == 0


@pytest.mark.parametrize("W,channels,frames", [
    (6001, 2, 300),     # chirp-z, L = 32768: 256 KiB of scratch per transform, 256 transforms per chunk
    (16384, 4, 70),     # direct, 2 x 32768 points per transform: 128 transforms per chunk, 2 pairs per frame
])
def test_batches_larger_than_the_scratch(torch_cuda, W, channels, frames):
    H = 61
    eng = engine(W, H, channels=channels)
    pcm = noise(W + (frames - 1) * H, channels, seed=frames)
    got = run(torch_cuda, eng, pcm)
    assert got.shape == (frames, channels // 2, W - 1, 2)
    check_against_truth(got, pcm, W, H, pairs=channels // 2)


@pytest.mark.parametrize("W", [6001, 19200])
def test_every_entry_point(torch_cuda, W):
    torch = torch_cuda
    from spectrogram_rs_amd import builtin_gradient
    H = W // 4
    eng = engine(W, H, gradient="viridis")
    assert eng.info.stft_kernel == 11 and eng.info.render_path == 0
    pcm = noise(W + 9 * H, 2, seed=W + 1)
    dev = torch.from_numpy(pcm).cuda().reshape(-1)
    mags = eng.stft_batch(dev)
    rows = mags.cpu().numpy()
    check_against_truth(rows, pcm, W, H)
    # half pairs: the float32 rows converted
    assert np.array_equal(eng.stft_batch_f16(dev).cpu().numpy(), mags.half().cpu().numpy())
    # two-kernel render: the pixel stage of the engine's own rows, and the oracle's pixels of them
    rgba = eng.render_batch(dev).cpu().numpy()
    own = eng.render_mags(mags[:, 0].contiguous()).cpu().numpy()
    assert np.array_equal(rgba[:, 0], own)
    assert np.array_equal(own, oracle.render_columns(rows[:, 0], int(SR), builtin_gradient("viridis")))
    # one frame from the host
    for t in (0, 7):
        assert np.array_equal(eng.process_one(pcm[t * H:t * H + W]), rows[t, 0]), t
    # a live ring tick
    ring = eng.live(W + 16 * H)
    assert ring.push(pcm, 2) == len(pcm)
    assert np.array_equal(ring.tick("mags"), rows[:, 0])


def test_fourier_mirror_takes_the_flag(torch_cuda):
    from spectrogram_rs_amd import SgxError
    from spectrogram_rs_amd.fourier import FastFourierTransform
    with pytest.raises(SgxError):
        FastFourierTransform(384000.0, 0.05)
    fft = FastFourierTransform(384000.0, 0.05, large_transforms=True)
    assert fft.num_input_samples() == 19200
    pcm = noise(19200, 2, seed=9)
    got = fft.process(pcm.reshape(-1))
    check_against_truth(got[None, None], pcm, 19200, 19200)
