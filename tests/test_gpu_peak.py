"""sgx_bands_peak_batch: peak-hold of sgx_bands_batch over groups of consecutive frames, and sgx_render_bands, through the C ABI.

A maximum is order-independent, so the yardstick is the library's own, unchanged sgx_bands_batch: every column must hold, bit for
bit, torch.amax over the same frames of bands_batch on the same engine (float equality stands in only where the bits differ by the
sign of a zero, which the header leaves open).  Checked on every case of tests/test_gpu_bands.py, fused against workspace route,
on splits, on a transient, at config 3's full size, and the colour stage against sgx_render_mags byte for byte."""
import ctypes as C

import numpy as np
import pytest

from spectrogram_rs_amd import SgxError, SpectrogramEngine, _lib
from test_gpu_bands import CASES, INTERPS, SR, make

pytestmark = pytest.mark.gpu

FRAMES_4096 = 5000   # W 2048: columns span many of the 1024 persistent workgroups, whose runs do not divide by the groups
FRAMES_LONG = 120    # every other window

# bands_peak_fused: 1 wherever sgx_bands_batch runs the fused 4096-point kernels (route 1: the W 2048 cases with bands_fused == 1) --
# but for SGX_FLAG_PAIRED_FRAMES, whose contexts were left on the workspace route (two frames of one transform, paired by their global
# index, may fall into different columns).  Every other case: 0.
PAIRED = {"w2048_h256_paired", "w2048_h200_paired"}
PEAK_FUSED = {name: int(kw.get("window_samples") == 2048 and fused == 1 and name not in PAIRED) for name, (kw, fused) in CASES.items()}


def same(a, b):
    """bit for bit; float equality only where the bits differ (the sign of a zero is unspecified)"""
    a, b = a.contiguous().view(-1).cpu().numpy(), b.contiguous().view(-1).cpu().numpy()
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    if np.array_equal(ua, ub):
        return True
    d = ua != ub
    return bool(np.all((a[d] == 0.0) & (b[d] == 0.0)))


def amax_groups(bands, group):
    """[F][...] -> [ceil(F / group)][...]: torch.amax over groups of consecutive frames"""
    import torch

    F = bands.shape[0]
    g = min(group, F)
    full = F // g
    parts = [bands[:full * g].reshape(full, g, *bands.shape[1:]).amax(1)]
    if full * g < F:
        parts.append(bands[full * g:].amax(0, keepdim=True))
    return torch.cat(parts, 0)


def frames_of(name):
    return FRAMES_4096 if CASES[name][0].get("window_samples") == 2048 else FRAMES_LONG


def groups_of(F):
    return [1, 2, 3, 7, 64, 977, F - 1, F, F + 5, 2 ** 40]


@pytest.mark.parametrize("interp", sorted(INTERPS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_definition_and_routes(name, interp):
    import torch

    eng = make(name, interp)
    F = frames_of(name)
    pcm = eng.white_noise(eng.W + (F - 1) * eng.H, seed=0x5EED0202)
    bands = eng.bands_batch(pcm)
    assert bands.shape[0] == F
    assert eng.bands_peak_fused == PEAK_FUSED[name], f"{name}: bands_peak_fused"
    split = make(name, interp, fused_render=False)
    assert split.bands_peak_fused == 0
    for group in groups_of(F):
        peak = eng.bands_peak_batch(pcm, group)
        cols = -(-F // group)
        assert peak.shape == (cols, eng.pairs, eng.R, 2), f"{name}/{interp}: group {group}"
        want = bands if group == 1 else amax_groups(bands, group)
        assert same(peak, want), f"{name}/{interp}: group {group} differs from amax over bands_batch"
        other = split.bands_peak_batch(pcm, group)
        assert same(peak, other), f"{name}/{interp}: group {group}: fused and workspace routes differ"
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr", "w2048_h200_mono", "w2048_ch4"])
def test_aligned_runs(name):
    """enough frames for the runs of the persistent workgroups to be rounded to whole columns of a small group (no combine pass),
    and a group next to it that is not"""
    import torch

    eng = make(name, "cubic")
    assert eng.bands_peak_fused == 1
    F = 200_000
    pcm = eng.white_noise(eng.W + (F - 1) * eng.H, seed=0x5EED0303)
    for group in (3, 4, 50):
        peak = eng.bands_peak_batch(pcm, group)
        step = 10_000 - 10_000 % group
        for f0 in range(0, F, step):
            n = min(step, F - f0)
            want = amax_groups(eng.bands_batch(pcm, first_frame=f0, max_frames=n), group)
            assert same(peak[f0 // group:f0 // group + want.shape[0]], want), f"{name}: group {group}, frames from {f0}"
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["w2048_h256_mono", "w2048_h256_lr", "w2048_h256_paired", "w2400_h93_mono", "w8192_h512"])
def test_splits(name):
    import torch

    eng = make(name, "cubic")
    F = 1000 if CASES[name][0].get("window_samples") == 2048 else FRAMES_LONG
    pcm = eng.white_noise(eng.W + (F - 1) * eng.H, seed=17)
    bands = eng.bands_batch(pcm)
    for group in (1, 5, 33):
        whole = eng.bands_peak_batch(pcm, group)
        assert same(whole, eng.bands_peak_batch(pcm, group)), f"{name}: a repeated call"
        # a range cut at multiples of the group, concatenated
        cuts = sorted({0, group * 2, group * 3, group * (F // group // 2), F})
        parts = [eng.bands_peak_batch(pcm, group, first_frame=a, max_frames=b - a) for a, b in zip(cuts, cuts[1:]) if b > a]
        assert same(torch.cat(parts, 0), whole), f"{name}: group {group}: pieces differ from the whole"
        # first_frame and max_frames that leave a short last column
        for first, count in [(3, 2 * group + 1), (F - group - 1, None), (F - 1, 100), (7, F)]:
            part = eng.bands_peak_batch(pcm, group, first_frame=first, max_frames=count)
            end = F if count is None else min(first + count, F)
            assert part.shape[0] == -(-(end - first) // group)
            assert same(part, amax_groups(bands[first:end], group)), f"{name}: group {group}: frames [{first}, {end})"
    torch.cuda.synchronize()


@pytest.mark.parametrize("extra", [dict(), dict(channels=2), dict(fused_render=False), dict(paired_frames=True)])
def test_transient_is_not_lost(extra):
    import torch

    W, H, F, group = 2048, 256, 640, 16
    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=H, device=0, **extra)
    # frames 98 .. 105 cover sample 256 * 105 + 200 (256 f <= s < 256 f + 2048), all of them inside column 6 = frames 96 .. 111 (and
    # whole pairs (2q, 2q + 1): with SGX_FLAG_PAIRED_FRAMES a frame shares its transform, and its rounding, with its partner)
    s = 256 * 105 + 200
    pcm = torch.zeros((W + (F - 1) * H) * eng.channels, dtype=torch.float32, device=eng.device)
    pcm[s * eng.channels:(s + 1) * eng.channels] = 1.0
    bands = eng.bands_batch(pcm)
    covering = [f for f in range(F) if H * f <= s < H * f + W]
    assert covering == list(range(98, 106)) and {f // group for f in covering} == {6}
    peak = eng.bands_peak_batch(pcm, group)
    torch.cuda.synchronize()
    assert peak.shape[0] == F // group
    top = float(peak[6].max())
    assert top == float(bands[covering].max()) and top > 0.0
    rest = torch.cat([peak[:6], peak[7:]], 0)
    assert bool((rest == 0.0).all()), "columns whose frames do not cover the impulse must be exactly 0"
    # raising the hop instead loses it: every sixteenth frame alone sees nothing of the impulse
    assert float(bands[::group].max()) == 0.0


@pytest.mark.parametrize("interp", sorted(INTERPS))
def test_full_size_config3(interp):
    """config 3's stream, 1e6 mono frames at W 2048 / H 256, in columns of 977 frames: against the maxima of sgx_bands_batch calls of
    9770 frames (ten columns, 80 MB) each"""
    import torch

    frames, W, H, group = 1_000_000, 2048, 256, 977
    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=H, device=0, interp=INTERPS[interp])
    assert eng.bands_peak_fused == 1
    pcm = eng.white_noise(W + (frames - 1) * H, seed=0x5EED0001)
    peak = eng.bands_peak_batch(pcm, group)
    assert peak.shape == (-(-frames // group), 1, eng.R, 2)
    step = 10 * group
    buf = torch.empty((step, 1, eng.R, 2), dtype=torch.float32, device=eng.device)
    want = torch.empty_like(peak)
    for f0 in range(0, frames, step):
        n = min(step, frames - f0)
        part = amax_groups(eng.bands_batch(pcm, first_frame=f0, max_frames=n, out=buf)[:n], group)
        want[f0 // group:f0 // group + part.shape[0]] = part
    torch.cuda.synchronize()
    assert same(peak, want)
    split = SpectrogramEngine(SR, window_samples=W, hop_samples=H, device=0, interp=INTERPS[interp], fused_render=False)
    assert same(split.bands_peak_batch(pcm, group), want)
    del pcm, peak, want
    torch.cuda.empty_cache()


def _schemes():
    ramp = np.array([[0, 0, 0], [40, 0, 80], [120, 0, 120], [200, 40, 60], [250, 120, 0], [255, 220, 60], [255, 255, 255]], np.uint8)
    return {
        "magma": (1, lambda e: e.set_builtin_gradient("magma")),
        "spline_spectral": (1, lambda e: e.set_builtin_scheme("spectral", stereo=False)),
        "diverging_red_blue": (2, lambda e: e.set_builtin_scheme("red_blue", stereo=True)),
        "ramp7": (1, lambda e: e.set_gradient(ramp)),
        "ramp7_diverging": (2, lambda e: e.set_gradient(ramp, stereo=True)),
    }


@pytest.mark.parametrize("scheme", sorted(_schemes()))
@pytest.mark.parametrize("W,H", [(2048, 256), (2400, 93)])
def test_colour(W, H, scheme):
    import torch

    channels, setup = _schemes()[scheme]
    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=H, channels=channels, device=0)
    setup(eng)
    F = 300
    pcm = eng.white_noise(W + (F - 1) * H, seed=0x5EED0404)
    want = eng.render_mags(eng.stft_batch(pcm).reshape(-1, eng.M, 2))
    bands = eng.bands_batch(pcm)
    got = eng.render_bands(bands.reshape(-1, eng.R, 2))
    torch.cuda.synchronize()
    assert got.shape == (F, eng.R, 4) and got.dtype == torch.uint8
    assert torch.equal(got, want), f"W {W} {scheme}: render_bands(bands_batch) differs from render_mags(stft_batch)"
    again = eng.render_bands(eng.bands_peak_batch(pcm, 1).reshape(-1, eng.R, 2))
    assert torch.equal(again, want), f"W {W} {scheme}: through bands_peak_batch(group = 1)"
    # a quiet stream reaches the low end of the ramp and the alpha table
    quiet = pcm * 1e-4
    assert torch.equal(eng.render_bands(eng.bands_batch(quiet).reshape(-1, eng.R, 2)), eng.render_mags(eng.stft_batch(quiet).reshape(-1, eng.M, 2)))


def test_contract():
    import torch

    eng = make("w2048_h256_mono", "cubic")
    F, group = 200, 7
    n = eng.W + (F - 1) * eng.H
    pcm = eng.white_noise(n, seed=23)
    full = eng.bands_peak_batch(pcm, group)
    cols = -(-F // group)
    lib, got = eng._lib, C.c_size_t(99)
    out = torch.empty((cols, 1, eng.R, 2), dtype=torch.float32, device=eng.device)
    dp, do = C.c_void_p(pcm.data_ptr()), C.c_void_p(out.data_ptr())
    # group = 0
    assert lib.sgx_bands_peak_batch(eng._ctx, dp, n, 0, F, 0, do, C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert got.value == 0
    with pytest.raises(SgxError):
        eng.bands_peak_batch(pcm, 0)
    # null buffers where columns exist
    got.value = 99
    assert lib.sgx_bands_peak_batch(eng._ctx, None, n, 0, F, group, do, C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert got.value == 0
    got.value = 99
    assert lib.sgx_bands_peak_batch(eng._ctx, dp, n, 0, F, group, None, C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert got.value == 0
    assert lib.sgx_bands_peak_batch(None, dp, n, 0, F, group, do, C.byref(got)) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_bands_peak_fused(None) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_render_bands(eng._ctx, None, 3, do) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_render_bands(eng._ctx, None, 0, None) == _lib.SGX_OK
    # trivial cases: SGX_OK and no columns, before any null check
    for args in [(eng.W - 1, 0, 10), (n, F, 10), (n, F + 7, 10), (n, 0, 0)]:
        got.value = 99
        assert lib.sgx_bands_peak_batch(eng._ctx, None, args[0], args[1], args[2], group, None, C.byref(got)) == _lib.SGX_OK
        assert got.value == 0
    # the count, and a NULL n_out
    assert lib.sgx_bands_peak_batch(eng._ctx, dp, n, 0, F, group, do, C.byref(got)) == _lib.SGX_OK
    assert got.value == cols
    assert lib.sgx_bands_peak_batch(eng._ctx, dp, n, F - 3, 100, 2, do, C.byref(got)) == _lib.SGX_OK
    assert got.value == 2
    assert lib.sgx_bands_peak_batch(eng._ctx, dp, n, 0, F, group, do, None) == _lib.SGX_OK
    torch.cuda.synchronize()
    assert same(out, full)
    assert eng.bands_peak_batch(pcm[:eng.W - 1], group).shape == (0, 1, eng.R, 2)
    # a non-default stream: the calls only enqueue (workspace and partial columns were grown by the calls above), on both routes
    split = make("w2048_h256_mono", "cubic", fused_render=False)
    assert same(split.bands_peak_batch(pcm, group), full)
    for e in (eng, split):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.cuda._sleep(400_000_000)
            other = e.bands_peak_batch(pcm, group)
            pending = not side.query()
        side.synchronize()
        assert pending, "the host must have run ahead of the stream"
        assert same(other, full)
    # a context only the multi-pass transform (kernel 11) serves: the workspace route
    big = make("w19200_large", "cubic")
    assert big.info.stft_kernel == 11 and big.bands_peak_fused == 0
    x = big.white_noise(big.W + 29 * big.H, seed=5)
    assert same(big.bands_peak_batch(x, 4), amax_groups(big.bands_batch(x), 4))
    torch.cuda.synchronize()
