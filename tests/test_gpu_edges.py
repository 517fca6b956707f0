"""Every transform route at the frame edges against the float64 truth (tests/edge_signals.py: the route table and the streams), all
through the C ABI.  Each row first asserts the kernel and render_path bits it names; then every frame of its edge stream is held to 1 x
the row's floor against its own truth (paired rows: against the pair's peak), frames with no non-zero windowed sample must come out
exactly zero, sub-ranges starting on target frames give the bytes of the full run, the half rows, fused pixels and fused bands follow
the float rows bit for bit, and NaN / inf at a frame's offset 0 and at offset W reach exactly the frames the reference says.
Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import edge_signals as es
from conftest import chirpz_bound, mags_error
from test_gpu_bands import two_call

pytestmark = pytest.mark.gpu

ROWS = [r.name for r in es.ROUTES]
_cache = {}


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


# Multiples of the row's floor its edge stream is held to (in the manner of conftest.KERNEL_BOUND and test_gpu_large.LARGE_BOUND): 1 x,
# with ONE measured exception.  The floors were measured on white noise, whose spectrum peaks well above its rounding noise.  An impulse
# pair has a flat spectrum, and on an (l, r) transform with one silent half (a pair on one channel, or a paired frame next to a silent
# partner) the silent half is the difference of two full-size float32 values: the rounding error against the peak is then larger than on
# noise, in every float32 FFT.  An independent float32 FFT (pocketfft, complex64) on these same streams reads up to 1.86 x (W 2048
# (l, r)), 2.04 x (W 8192), 2.9 x (chirp-z W 1852) and 3.8 x (W 65537).  The rows below measured above 1 x on the MI355X, the worst
# 2.21 x (W 65537, chirp-z over kernel 11), 2.10 x (K16, 8 channels, H 300), 1.85 x (chirp-z W 1102 (l, r)), 1.71 x (K1 (l, r), H 58);
# every real-input row holds 1 x.  A misread of an edge sample reads >= 100 x (tests/test_edge_signals.py).
EDGE_BOUND = {"default": 1.0, "flat spectra": 2.5}
FLAT_SPECTRUM_ROWS = {
    "k1_lr_h256", "k1_lr_h58", "k1_paired_mono", "k1_ch8", "k16_lr_h512", "k16_lr_h300", "k16_ch8_h512", "k16_ch8_h300",
    "k16_mono_h512", "k48_lr", "k48_paired_mono", "mixed_w2400_generic", "mixed_w2400_ch4", "mixed_w4096_lr", "mixed_w735_runtime_lr",
    "chirpz_w1102_lr", "chirpz_w1852_lr", "bluestein_w1102", "generic_w2048_lr", "large_w19200_lr", "large_w6001_chirp_lr",
    "large_w65537_chirp_lr", "large_w6001_chunks"}


def bound(r):
    if r.name in FLAT_SPECTRUM_ROWS:
        return EDGE_BOUND["flat spectra"]
    return chirpz_bound(r.W) if r.kernel == 4 else EDGE_BOUND["default"]


def case(torch, name):
    """(route, stream, engine, device stream, full stft_batch rows), built once per row"""
    if name not in _cache:
        r = es.ROUTE[name]
        s = es.build_stream(r)
        eng = engine(r, gradient="viridis")
        dev = to_dev(torch, r, s.pcm)
        got = eng.stft_batch(dev).cpu().numpy()
        _cache[name] = (r, s, eng, dev, got)
    return _cache[name]


@pytest.mark.parametrize("name", ROWS)
def test_route(torch_cuda, name):
    r, _, eng, _, _ = case(torch_cuda, name)
    info = eng.info
    assert info.stft_kernel == r.kernel, (name, info.stft_kernel)
    assert info.render_path & r.bits_set == r.bits_set and info.render_path & r.bits_clear == 0, (name, info.render_path)
    if r.bands_fused is not None:
        assert eng.bands_fused == r.bands_fused, (name, eng.bands_fused)


@pytest.mark.parametrize("name", ROWS)
def test_every_frame_against_the_truth(torch_cuda, name):
    r, s, _, _, got = case(torch_cuda, name)
    W = r.W
    assert got.shape == (s.frames, r.pairs, W - 1, 2)
    worst, where, silent_frames = 0.0, None, 0
    truth_cache = {}

    def truth(t, p):
        if (t, p) not in truth_cache:
            truth_cache[(t, p)] = es.truth_frame(es.frame_lr(s.frame(t), p), W)
        return truth_cache[(t, p)]

    for t in range(s.frames):
        silent = es.windowed_silent(s.frame(t), W)
        for p in range(r.pairs):
            ref = truth(t, p)
            quiet = bool(silent[2 * p:2 * p + 2].all()) if r.channels > 1 else bool(silent[0])
            if r.paired:
                q = t ^ 1
                partner = float(np.abs(truth(q, 0)).max()) if q < s.frames else 0.0
                if quiet and partner == 0.0:
                    assert not got[t, p].any(), (name, t, "a silent transform must be exactly zero")
                    silent_frames += 1
                    continue
                err = es.pair_error(got[t, p], ref, r.floor, partner)
            else:
                if quiet:   # no non-zero windowed sample: exactly zero, whatever the kernel read around it
                    assert not got[t, p].any(), (name, t, p, "a silent frame must be exactly zero")
                    silent_frames += 1
                    continue
                err = mags_error(got[t, p], ref, r.floor)
            if err > worst:
                worst, where = err, (t, p)
    assert silent_frames >= 1
    print(f"EDGE-RATIO {name} worst {worst:.4f} at {where} (bound {bound(r)}), {silent_frames} silent frame-pairs exactly zero")
    assert worst <= bound(r), (name, where, worst)


@pytest.mark.parametrize("name", ROWS)
def test_sub_ranges_from_target_frames(torch_cuda, name):
    r, s, eng, dev, got = case(torch_cuda, name)
    tf = [sl.frame for sl in s.target_slots()]
    even = next(t for t in tf[1:] if t % 2 == 0)
    odd = next((t for t in tf if t % 2 == 1), None)
    calls = [(even, 1), (even, 3), (tf[-1], 1)]
    if odd is not None:
        calls += [(odd, 1), (odd, 4), (odd, None)]
    for first, count in calls:
        part = eng.stft_batch(dev, first_frame=first, max_frames=count).cpu().numpy()
        end = s.frames if count is None else min(s.frames, first + count)
        assert np.array_equal(part, got[first:end]), (name, first, count)


@pytest.mark.parametrize("name", ROWS)
def test_half_rows_pixels_and_bands(torch_cuda, name):
    torch = torch_cuda
    r, s, eng, dev, got = case(torch, name)
    rows = torch.from_numpy(got).cuda()
    assert torch.equal(eng.stft_batch_f16(dev), rows.half()), name
    if eng.info.render_path & 1:   # one fused PCM-to-pixel kernel: the pixels of the rows, byte for byte
        px = eng.render_batch(dev)
        if r.kernel == 9 and r.channels <= 2 and not eng.info.render_path & 8:
            # (the 4800-point kernel writes rows only: the fused pixels are the composite-radix kernel's, as in
            # test_gpu_parity.py::test_app_point_4800_point_kernel -- the pixels of the rows of a SGX_FLAG_MIXED_GENERIC context)
            rows = engine(r, mixed_generic=True).stft_batch(dev)
        own = eng.render_mags(rows.reshape(-1, eng.M, 2).contiguous())
        assert torch.equal(px.reshape(own.shape), own), name
    if eng.bands_fused:            # one fused PCM-to-bands kernel: stft_batch + magnitude_in, bit for bit
        bands = eng.bands_batch(dev)
        mags, ref = two_call(eng, dev)
        assert np.array_equal(mags.cpu().numpy(), got)
        assert np.array_equal(bands.cpu().numpy().view(np.uint32), ref.cpu().numpy().view(np.uint32)), name


# one row per kernel family (and per way of loading more rows than a frame holds: K1R's slide, two-frame workgroups, K16's row pairs)
NON_FINITE_ROWS = ["k1r_h256", "k1r_h100", "k1_lr_h58", "k1_paired_mono", "k1_ch8", "k16_mono_h512", "k16_ch8_h512", "k16_lr_h300",
                   "k48_lr", "k48_paired_mono", "mixed_w2205_real", "mixed_w2400_real", "mixed_w2400_ch4", "mixed_w735_runtime_lr",
                   "chirpz_w1102_real", "chirpz_w1852_lr", "bluestein_w1102", "generic_w256_mono", "generic_w2048_lr",
                   "large_w10290_mono", "large_w6001_chirp_lr"]


@pytest.mark.parametrize("name", NON_FINITE_ROWS)
def test_non_finite_samples_at_the_edges(torch_cuda, name):
    # the rule of test_gpu_parity.py::test_non_finite_and_extreme_samples at the edges: a NaN / inf at offset 0 of a frame makes that
    # frame non-finite (the reference computes 0 * NaN); a NaN at offset W, the first sample after the window, leaves that frame
    # bit-identical; on paired rows the partner frame of the same transform may turn non-finite too
    torch = torch_cuda
    r = es.ROUTE[name]
    W, H, C = r.W, r.H, r.channels
    F = 12
    n = (F - 1) * H + W
    import oracle
    clean = (oracle.white_noise(n * C, seed=W + C) * np.float32(0.1)).reshape(n, C)
    bad = clean.copy()
    hits = [(0, 0, np.inf), (2 * H, C - 1, np.nan), (5 * H + W, 0, np.nan), ((F - 2) * H + W, C - 1, np.nan)]
    touched = np.zeros((F, r.pairs), bool)
    for p, c, v in hits:
        bad[p, c] = v
        for t in range(F):
            if t * H <= p < t * H + W:
                touched[t, c // 2 if C > 1 else 0] = True
    assert touched[0].any() and touched[2].any() and not touched[5].any()
    eng = engine(r)
    good_m = eng.stft_batch(to_dev(torch, r, clean)).cpu().numpy()
    bad_m = eng.stft_batch(to_dev(torch, r, bad)).cpu().numpy()
    allowed = touched.copy()
    if r.paired:
        allowed |= np.array([touched[min(t ^ 1, F - 1)] for t in range(F)])
    for t in range(F):
        for p in range(r.pairs):
            if touched[t, p]:
                assert not np.isfinite(bad_m[t, p]).all(), (name, t, p, "must be non-finite")
            elif not allowed[t, p]:
                assert np.array_equal(bad_m[t, p], good_m[t, p]), (name, t, p, "must be bit-identical")
