"""Device memory that is replaced or regrown under a living context, and contexts that come and go (csrc/device_buffer.hpp: every table,
workspace and scratch is a buffer owned by the object that uses it).  Each sequence below makes a context free and allocate a buffer it
has already used -- a palette uploaded again, the range-table cache replaced, scratch and workspace regrown, tables built by a later
call -- and every result is compared, bit for bit, with a FRESH context that took only the final configuration and made only that call;
never with the same context's earlier output.  The last test creates and destroys one context per transform family three times over.
Smallest shapes that reach each buffer (rows = 8: small pixel tables).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import length_sweep as ls

pytestmark = pytest.mark.gpu

W, H = 2048, 256
RAMP = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], 1).astype(np.uint8)   # a 256-entry ramp, no builtin's
RANGES_A = np.array([[40, 80], [80, 300], [300, 301], [1000, 5000], [5000, 20000]], np.float32)
RANGES_B = np.array([[32, 64], [64, 4000], [4000, 22000]], np.float32)                                      # (a different count)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def noise(torch, n_samples, channels, seed):
    x = np.random.default_rng(seed).standard_normal((n_samples, channels)).astype(np.float32) * 0.25
    return torch.from_numpy(x).cuda()


def engine(**kw):
    from spectrogram_rs_amd import SpectrogramEngine
    kw.setdefault("rows", 8)
    return SpectrogramEngine(48000.0, device=0, **kw)


def fresh(call, **kw):
    """what `call` returns on a context that has done nothing else"""
    eng = engine(**kw)
    try:
        return call(eng).cpu().numpy()
    finally:
        eng.close()


def test_a_palette_uploaded_again_gives_the_pixels_of_a_fresh_context(torch_cuda):
    torch = torch_cuda
    kw = dict(window_samples=W, hop_samples=H, channels=1)
    pcm = noise(torch, W + 39 * H, 1, 1)

    def ramp(e):
        e.set_gradient(RAMP)
        return e.render_batch(pcm)

    def cool(e):
        e.set_builtin_scheme("cool", stereo=True)
        return e.render_batch(pcm)

    eng = engine(**kw)
    first = ramp(eng).cpu().numpy()
    assert eng.info.render_path & 1                       # the fused pixels: they read the ramp's seed table
    diverging = cool(eng).cpu().numpy()                   # a segment palette: other tables, the seed table gone
    assert not eng.info.render_path & 1
    again = ramp(eng).cpu().numpy()
    eng.close()
    assert first.shape == (40, 1, 8, 4)
    assert np.array_equal(first, fresh(ramp, **kw))
    assert np.array_equal(diverging, fresh(cool, **kw)) and not np.array_equal(diverging, first)
    assert np.array_equal(again, first) and np.array_equal(again, fresh(ramp, **kw))


def test_a_range_set_replaced_and_restored_gives_the_bands_of_a_fresh_context(torch_cuda):
    torch = torch_cuda
    kw = dict(window_samples=W, hop_samples=H, channels=1)
    pcm = noise(torch, W + 39 * H, 1, 2)
    eng = engine(**kw)
    mags = eng.stft_batch(pcm)[:, 0].contiguous()
    a1 = eng.magnitude_in(mags, RANGES_A).cpu().numpy()
    b = eng.magnitude_in(mags, RANGES_B).cpu().numpy()
    a2 = eng.magnitude_in(mags, RANGES_A).cpu().numpy()
    eng.close()
    fresh_a = fresh(lambda e: e.magnitude_in(mags, RANGES_A), **kw)
    assert a1.shape == (40, 5, 2) and b.shape == (40, 3, 2)
    assert np.array_equal(a1, fresh_a) and np.array_equal(a2, fresh_a)
    assert np.array_equal(b, fresh(lambda e: e.magnitude_in(mags, RANGES_B), **kw))


def test_scratch_that_regrows_gives_the_output_of_a_fresh_context(torch_cuda):
    torch = torch_cuda
    kw = dict(window_samples=W, hop_samples=H, channels=8)
    pcm = noise(torch, W + 39 * H, 8, 3)
    eng = engine(**kw)
    # the pair planes of a stream of more than two channels: sized by the call's sample range
    few = eng.stft_batch(pcm, max_frames=3).cpu().numpy()
    many = eng.stft_batch(pcm).cpu().numpy()
    # the partial columns of the fused peak hold: sized by the compute units in force
    assert eng.bands_peak_fused
    eng.set_cu_limit(2)
    narrow = eng.bands_peak_batch(pcm, 4).cpu().numpy()
    eng.set_cu_limit(0)
    n_cu = eng.cu_limit
    wide = eng.bands_peak_batch(pcm, 4).cpu().numpy()
    eng.close()
    assert n_cu > 2 and few.shape == (3, 4, W - 1, 2) and many.shape == (40, 4, W - 1, 2) and wide.shape == (10, 4, 8, 2)
    assert np.array_equal(few, fresh(lambda e: e.stft_batch(pcm, max_frames=3), **kw))
    assert np.array_equal(many, fresh(lambda e: e.stft_batch(pcm), **kw))

    def at_two(e):
        e.set_cu_limit(2)
        return e.bands_peak_batch(pcm, 4)

    assert np.array_equal(narrow, fresh(at_two, **kw))
    assert np.array_equal(wide, fresh(lambda e: e.bands_peak_batch(pcm, 4), **kw))


def test_a_workspace_that_grows_and_tables_built_by_a_call_give_the_output_of_a_fresh_context(torch_cuda):
    torch = torch_cuda
    # W 1000 (mixed radix), two kernels: the rows of a chunk of frames go through the workspace
    kw = dict(window_samples=1000, hop_samples=250, channels=2, fused_render=False)
    pcm = noise(torch, 1000 + 29 * 250, 2, 4)
    eng = engine(**kw)
    assert eng.info.stft_kernel == 6 and not eng.info.render_path & 1
    two = eng.render_batch(pcm, max_frames=2).cpu().numpy()
    thirty = eng.render_batch(pcm).cpu().numpy()
    eng.close()
    assert two.shape == (2, 1, 8, 4) and thirty.shape == (30, 1, 8, 4)
    assert np.array_equal(two, fresh(lambda e: e.render_batch(pcm, max_frames=2), **kw))
    assert np.array_equal(thirty, fresh(lambda e: e.render_batch(pcm), **kw))
    # W 2400 stereo: the inverse's tables are built by the first istft_batch and serve the second
    kw = dict(window_samples=2400, hop_samples=600, channels=2)
    pcm = noise(torch, 2400 + 5 * 600, 2, 5)
    eng = engine(**kw)
    spec = eng.stft_batch_complex(pcm)
    once = eng.istft_batch(spec).cpu().numpy()
    twice = eng.istft_batch(spec).cpu().numpy()
    eng.close()
    fresh_pcm = fresh(lambda e: e.istft_batch(spec), **kw)
    assert once.shape == (2400 + 5 * 600, 2)
    assert np.array_equal(once, fresh_pcm) and np.array_equal(twice, fresh_pcm)


# The smallest window whose chirp-z runs the radix-4 ladder of stft_bluestein.hip by default: a prime factor above 7 in 2W and a
# convolution shorter than the composite stages take (length_sweep.CHIRP_STAGES_MIN_L: W < 86)
W_LADDER = min(w for w in range(4, 86) if ls.chirp_served(w) and ls.chirp_length(w) < ls.CHIRP_STAGES_MIN_L)
W_LARGE = min(e.W for e in ls.LARGE_DIRECT)   # a length only SGX_FLAG_LARGE_TRANSFORM serves
# (name, window, channels, flags, stft_kernel, render_path bit 2: a compile-time plan of the composite stages -- set by chirp-z through
# them, clear on the ladder; None: not asked)
FAMILIES = [
    ("generic", 128, 2, {}, 0, None),
    ("4096-point (l, r)", 2048, 2, {}, 2, None),
    ("real-input", 2048, 1, {}, 2, None),
    ("4800", 2400, 2, {}, 9, None),
    ("mixed", 1000, 2, {}, 6, None),
    ("chirp-z", 1031, 2, {}, 4, True),
    ("Bluestein", W_LADDER, 2, {}, 4, False),
    ("16384", 8192, 2, {}, 10, None),
    ("multi-pass", W_LARGE, 2, {"large_transforms": True}, 11, None),
]


def test_every_family_is_created_and_destroyed_three_times_over(torch_cuda):
    torch = torch_cuda
    assert W_LADDER == 11 and W_LARGE > ls.MIX_MAX_P // 2
    first_round = {}
    for rnd in range(3):
        for name, w, channels, flags, kernel, bit2 in FAMILIES:
            h = 256 if w == 2048 else w // 3 + 1
            pcm = noise(torch, w + 2 * h, channels, w)
            eng = engine(window_samples=w, hop_samples=h, channels=channels, **flags)
            assert eng.info.stft_kernel == kernel, name
            if bit2 is not None:
                assert bool(eng.info.render_path & 4) == bit2, name
            if name == "real-input":
                assert eng.info.render_path & 8
            rows = eng.stft_batch(pcm).cpu().numpy()
            eng.close()
            assert rows.shape == (3, 1, w - 1, 2) and np.isfinite(rows).all() and rows.any(), name
            assert np.array_equal(rows, first_round.setdefault(name, rows)), (name, rnd)
