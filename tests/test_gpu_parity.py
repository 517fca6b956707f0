"""Parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on the same
seeded inputs, against the committed golden fixtures, and -- at sizes the oracle cannot reach --
through size-independent properties.  Run with -m gpu on an MI355X."""
import os

import numpy as np
import pytest

import edge_signals as es
import oracle
from conftest import FLOOR_K16, FLOOR_WIDE     # floors of the kernels outside BASELINE configs 1-3 (tests/conftest.py: measured need)

pytestmark = pytest.mark.gpu

W, H, SR, R = 2048, 256, 48000, 1024
M = W - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def engine(**kw):
    from spectrogram_rs_amd import SpectrogramEngine
    return SpectrogramEngine(48000.0, **kw)


def oracle_prime_factor(n):
    """largest prime factor of n (the float32 oracle evaluates each prime factor p as a plain p-term sum)"""
    p, big = 2, 1
    while p * p <= n:
        while n % p == 0:
            big, n = p, n // p
        p += 1
    return max(big, n) if n > 1 else big


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().reshape(-1)


# ---- the transform -----------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["default", "paired", "complex", "generic", "generic_paired"])
@pytest.mark.parametrize("channels", [1, 2])
def test_stft_batch_matches_oracle(torch_cuda, mags_err, variant, channels):
    # every kernel that can serve W = 2048: workgroup-per-transform (default; a mono stream: the real-input kernel, "paired": two
    # frames per transform, "complex": every frame its (s, s) transform) and the generic power-of-two kernel
    torch = torch_cuda
    kw = {"default": {}, "paired": {"paired_frames": True}, "complex": {"complex_mono": True}, "generic": {"force_generic": True},
          "generic_paired": {"force_generic": True, "paired_frames": True}}[variant]
    eng = engine(window_samples=W, hop_samples=H, channels=channels, **kw)
    assert eng.info.stft_kernel == {"default": 2, "paired": 2, "complex": 2, "generic": 0}[variant.split("_")[0]]
    assert bool(eng.info.render_path & 8) == (variant == "default" and channels == 1)
    n = W + H * 130 + 77
    pcm = oracle.white_noise(n * channels, seed=11 + channels)
    got = eng.stft_batch(to_dev(torch, pcm)).cpu().numpy()
    ref32 = oracle.stream_process(pcm, channels, W, H, threads=8)
    ref64 = np.stack([oracle.np_truth_frame(
        (np.stack([pcm[t * H:t * H + W]] * 2, 1) if channels == 1 else pcm.reshape(-1, 2)[t * H:t * H + W]), W)
        for t in range(131)])
    assert got.shape == ref32.shape == (131, 1, M, 2)
    assert mags_err(got[:, 0], ref64) <= 1.0             # EVERY frame against the float64 truth, at 1 x north_star's tolerance
    assert mags_err(got, ref32) <= 2.0                   # two float32 FFTs, each within tolerance of the truth
    if channels == 1:
        # mono -> (s, s): both columns are |S^[k]| (computed by different float32 expressions in the
        # reference too, fft.rs:87-88, so equal to rounding, not bit for bit)
        assert mags_err(got[..., 0:1], got[..., 1:2].astype(np.float64)) <= 1.0


def test_golden_frames_through_the_abi(torch_cuda, gold, mags_err):
    torch = torch_cuda
    eng = engine(window_samples=W, hop_samples=H, channels=1)
    for name in ("config1_sweep.npz", "noise_frames.npz"):
        g = gold(name)
        for s, exp in zip(g["input"], g["expected_f64"]):
            got = eng.stft_batch(to_dev(torch, s)).cpu().numpy()
            assert got.shape == (1, 1, M, 2)
            assert mags_err(got[0, 0], exp) <= 1.0


@pytest.mark.parametrize("Wt,Ht,ch", [(8192, 512, 8), (8192, 300, 4), (8192, 1024, 6), (1024, 93, 2), (64, 16, 1), (4, 1, 2), (2048, 58, 2)])
def test_other_sizes_and_channel_pairs(torch_cuda, mags_err, Wt, Ht, ch):
    # config 4 (16384-point, 8 interleaved channels = 4 pairs; hops that are / are not multiples of 512: the de-interleaved
    # planes are stored row-paired for 16-byte sample reads only for the former) and assorted power-of-two windows
    torch = torch_cuda
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=ch)
    n = Wt + Ht * 9 + 3
    pcm = oracle.white_noise(n * ch, seed=5)
    got = eng.stft_batch(to_dev(torch, pcm)).cpu().numpy()
    ref = oracle.stream_process(pcm, ch, Wt, Ht, threads=8)
    assert got.shape == ref.shape == (oracle.num_frames(n, Wt, Ht), max(ch // 2, 1), Wt - 1, 2)
    assert got.shape[0] >= 10
    assert mags_err(got, ref) <= 2.0


@pytest.mark.parametrize("ch,kw", [(2, {}), (4, {}), (1, {}), (1, {"paired_frames": True}), (1, {"complex_mono": True})])
def test_sliding_windows_over_long_runs(torch_cuda, mags_err, ch, kw):
    # At H = 256 the 4096-point kernels slide their sample window in registers: a persistent workgroup loads a whole window only for the
    # FIRST transform of its run and one new row per transform after that.  A launch of a few hundred frames gives every workgroup one
    # transform -- the sliding code never runs.  Here every workgroup owns ~6 consecutive transforms: every frame must equal, bit for bit,
    # the same frame computed alone (a one-frame launch: whole-window load) and, on a sample, the oracle's.
    torch = torch_cuda
    F = 6151
    eng = engine(window_samples=W, hop_samples=H, channels=ch, gradient="viridis", **kw)
    pcm = oracle.white_noise(((F - 1) * H + W) * ch, seed=77 + ch)
    dev = to_dev(torch, pcm)
    full = eng.stft_batch(dev)
    half = eng.stft_batch_f16(dev)
    pix = eng.render_batch(dev)
    assert full.shape[0] == F
    rng = np.random.default_rng(3)
    for t in sorted(set([0, 1, 2, 5, 6, 7, F - 2, F - 1] + [int(v) for v in rng.integers(0, F, 24)])):
        cnt = 2 if (ch == 1 and t + 1 < F) else 1          # mono kernels take frames in pairs: an even start, two frames
        t0 = t - (t & 1) if ch == 1 else t
        assert torch.equal(eng.stft_batch(dev, first_frame=t0, max_frames=cnt), full[t0:t0 + cnt]), t
        assert torch.equal(eng.stft_batch_f16(dev, first_frame=t0, max_frames=cnt), half[t0:t0 + cnt]), t
        assert torch.equal(eng.render_batch(dev, first_frame=t0, max_frames=cnt), pix[t0:t0 + cnt]), t
    pick = np.unique(np.concatenate([[0, 1, 6, 7, F - 1], rng.integers(0, F, 40)]))
    got = full.cpu().numpy()[pick]
    ref = np.stack([oracle.stream_process(pcm[t * H * ch:(t * H + W) * ch], ch, W, H)[0] for t in pick])
    assert mags_err(got, ref) <= 2.0


@pytest.mark.parametrize("ch,Ht", [(4, 256), (8, 256), (8, 100), (6, 512)])
def test_4096_point_kernel_on_interleaved_channel_pairs(torch_cuda, mags_err, gradients, ch, Ht):
    # more than two channels at W = 2048: the pairs are split into planes and each runs the two-channel kernel (transform,
    # half rows and the fused pixel path alike); sub-ranges give the same bytes; an odd stream offset too
    torch = torch_cuda
    eng = engine(window_samples=W, hop_samples=Ht, channels=ch)
    assert eng.info.stft_kernel == 2
    n = W + 13 * Ht + 7
    pcm = oracle.white_noise(n * ch, seed=ch * 100 + Ht)
    dev = to_dev(torch, pcm)
    got = eng.stft_batch(dev).cpu().numpy()
    ref = oracle.stream_process(pcm, ch, W, Ht, threads=8)
    assert got.shape == ref.shape == (14, ch // 2, M, 2)
    assert mags_err(got, ref, FLOOR_WIDE) <= 1.0
    for first, cnt in ((1, 5), (13, 1), (4, 10)):
        assert np.array_equal(eng.stft_batch(dev, first_frame=first, max_frames=cnt).cpu().numpy(), got[first:first + cnt])
    shifted = torch.empty(dev.numel() + 1, dtype=dev.dtype, device=dev.device)
    shifted[1:] = dev
    assert np.array_equal(eng.stft_batch(shifted[1:]).cpu().numpy(), got)
    assert torch.equal(eng.stft_batch_f16(dev), torch.from_numpy(got).cuda().to(torch.float16))
    eng.set_gradient(gradients["viridis"])
    px = eng.render_batch(dev).cpu().numpy()
    own = oracle.render_columns(got.reshape(-1, M, 2), SR, gradients["viridis"])
    assert px.shape == (14, ch // 2, R, 4) and np.array_equal(px.reshape(own.shape), own)


@pytest.mark.parametrize("ch,paired", [(2, False), (1, True), (1, False), (4, False)])
@pytest.mark.parametrize("variant", ["tuned", "composite"])
def test_app_point_4800_point_kernel(torch_cuda, mags_err, gradients, ch, paired, variant):
    # The application's own window (48 kHz x 0.05 s = W 2400, 2W = 4800 = 16 x 20 x 15; hop 93 = (2 / 1024) s): the tuned
    # workgroup-per-transform kernel (default for one and two channels; more channels run the composite-radix kernel of any smooth
    # length) and that kernel itself (SGX_FLAG_MIXED_GENERIC), each against the oracle -- rows, half rows, pixel columns
    torch = torch_cuda
    Wt, Ht = 2400, 93
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=ch, paired_frames=paired, mixed_generic=(variant == "composite"),
                 gradient="viridis")
    assert eng.info.stft_kernel == (9 if variant == "tuned" else 6)
    # 768 persistent workgroups on a 256-CU device: mono pairs -> 951 jobs, two per workgroup for some; stereo -> 3 per workgroup.
    # A mono stream of an ODD number of frames: the last pair has no second frame (its imaginary part is zero, its row is not stored)
    frames = 1901 if ch == 1 else 1900
    n = Wt + (frames - 1) * Ht + 17
    pcm = oracle.white_noise(n * ch, seed=300 + ch)
    dev = to_dev(torch, pcm)
    got = eng.stft_batch(dev).cpu().numpy()
    ref = oracle.stream_process(pcm, ch, Wt, Ht, threads=8)
    assert got.shape == ref.shape == (frames, max(ch // 2, 1), Wt - 1, 2)
    assert mags_err(got, ref, FLOOR_WIDE) <= 2.0
    lr = pcm.reshape(-1, ch)
    for f in (0, 7, frames - 1):
        truth = oracle.np_truth_frame(np.stack([lr[f * Ht:f * Ht + Wt, 0], lr[f * Ht:f * Ht + Wt, min(1, ch - 1)]], 1), Wt)
        assert mags_err(got[f, 0], truth, FLOOR_WIDE) <= 1.0
    for _ in range(3):   # the same bytes every time
        assert np.array_equal(eng.stft_batch(dev).cpu().numpy(), got)
    for first, cnt in ((1, 4), (6, 3), (frames - 1, 1), (3, 1001)):   # sub-ranges give the same bytes (mono pairs by global index)
        assert np.array_equal(eng.stft_batch(dev, first_frame=first, max_frames=cnt).cpu().numpy(), got[first:first + cnt])
    assert torch.equal(eng.stft_batch_f16(dev), torch.from_numpy(got).cuda().to(torch.float16))
    assert torch.equal(eng.stft_batch_f16(dev, first_frame=5, max_frames=77), torch.from_numpy(got[5:82]).cuda().to(torch.float16))
    # PCM -> RGBA.  One kernel from PCM to pixels is the composite-radix kernel's (the tuned kernel writes rows only), so a default
    # context renders what a SGX_FLAG_MIXED_GENERIC context renders; the two-kernel route (SGX_FLAG_NO_FUSED_RENDER) runs the pixel
    # stage on the context's own rows.  Either way: the oracle's pixel stage on the magnitudes that were rendered, byte for byte
    px = eng.render_batch(dev).cpu().numpy()
    assert px.shape == (frames, max(ch // 2, 1), R, 4)
    assert bool(eng.info.render_path & 1)
    assert np.array_equal(eng.render_batch(dev, first_frame=3, max_frames=50).cpu().numpy(), px[3:53])
    split = engine(window_samples=Wt, hop_samples=Ht, channels=ch, paired_frames=paired, mixed_generic=(variant == "composite"),
                   gradient="viridis", fused_render=False)
    own = oracle.render_columns(got.reshape(-1, Wt - 1, 2), SR, gradients["viridis"])
    assert np.array_equal(split.render_batch(dev).cpu().numpy().reshape(own.shape), own)
    split.close()
    if variant == "composite" or ch > 2:
        assert np.array_equal(px.reshape(own.shape), own)
    else:
        comp = engine(window_samples=Wt, hop_samples=Ht, channels=ch, paired_frames=paired, mixed_generic=True, gradient="viridis")
        assert np.array_equal(comp.render_batch(dev).cpu().numpy(), px)
        comp.close()
    eng.close()


@pytest.mark.parametrize("ch,variant", [(8, "tuned"), (6, "tuned"), (2, "tuned"), (1, "tuned"), (1, "tuned_paired"), (8, "generic")])
def test_config4_16384_point_kernel(torch_cuda, mags_err, ch, variant):
    # BASELINE config 4: W 8192 / P 16384, hop 512, interleaved channel pairs; the tuned kernel (32 x 32 x 16 in one 512-thread workgroup,
    # stft16384_w.hip: stft_kernel 10) and the generic kernel, each against the oracle
    torch = torch_cuda
    Wt, Ht = 8192, 512
    # (a mono stream: by default every frame its own (s, s) transform -- the tuned kernel on a duplicated plane --, "_paired": two frames
    # per transform, SGX_FLAG_PAIRED_FRAMES)
    paired = variant.endswith("_paired")
    variant = variant.split("_")[0]
    force_generic = variant == "generic"
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=ch, force_generic=force_generic, paired_frames=paired)
    assert eng.info.stft_kernel == {"tuned": 10, "generic": 0}[variant]
    n = Wt + 21 * Ht + 9
    pcm = oracle.white_noise(n * ch, seed=40 + ch)
    dev = to_dev(torch, pcm)
    got = eng.stft_batch(dev).cpu().numpy()
    ref = oracle.stream_process(pcm, ch, Wt, Ht, threads=8)
    assert got.shape == ref.shape == (22, max(ch // 2, 1), Wt - 1, 2)
    assert mags_err(got, ref) <= 2.0
    lr = pcm.reshape(-1, ch)
    truth = oracle.np_truth_frame(np.stack([lr[5 * Ht:5 * Ht + Wt, 0], lr[5 * Ht:5 * Ht + Wt, min(1, ch - 1)]], 1), Wt)
    assert mags_err(got[5, 0], truth) <= 1.0
    for _ in range(4):   # the same bytes every time (a store hazard once corrupted a few pieces of a row, now and then)
        assert np.array_equal(eng.stft_batch(dev).cpu().numpy(), got)
    for first, cnt in ((1, 4), (6, 3), (21, 1)):   # sub-ranges give the same bytes (mono pairs by global index)
        assert np.array_equal(eng.stft_batch(dev, first_frame=first, max_frames=cnt).cpu().numpy(), got[first:first + cnt])
    if ch == 8:
        # a stream that is 8- but not 16-byte aligned: same bytes
        shifted = torch.empty(dev.numel() + 2, dtype=dev.dtype, device=dev.device)
        shifted[2:] = dev
        assert shifted[2:].data_ptr() % 16 == 8
        assert np.array_equal(eng.stft_batch(shifted[2:]).cpu().numpy(), got)
    if variant != "generic" and ch >= 6:
        # more jobs than persistent workgroups (142 hop positions x 4 pairs = 568 > 512): every workgroup runs several jobs with
        # different data -- a stale read of what the previous job left (the kernel re-uses its LDS image, its prefetch registers and the
        # pending row across jobs) would show here
        # 530 hop positions = 2 120 jobs: also past the size from which the kernel hands every XCD its own eighth of the jobs
        for hops in (142, 530):
            pcm2 = oracle.white_noise((Wt + (hops - 1) * Ht) * ch, seed=77 + hops)
            dev2 = to_dev(torch, pcm2)
            got2 = eng.stft_batch(dev2).cpu().numpy()
            ref2 = oracle.stream_process(pcm2, ch, Wt, Ht, threads=8)
            assert got2.shape == ref2.shape == (hops, ch // 2, Wt - 1, 2) and mags_err(got2, ref2) <= 2.0
        # a sub-range cuts the stream into other runs of hop positions (the sliding window starts somewhere else): the same bytes
        assert np.array_equal(eng.stft_batch(dev2, first_frame=7, max_frames=300).cpu().numpy(), got2[7:307])
    if variant == "tuned" and not paired and ch <= 2:
        # hop 512 = the thread stride of the kernel's first pass: a workgroup takes a RUN of hop positions of one pair and keeps the
        # window in registers (one new sample per thread and transform).  1 100 hop positions on 256 workgroups: runs of 5
        hops = 1100
        pcm2 = oracle.white_noise((Wt + (hops - 1) * Ht) * ch, seed=91 + ch)
        dev2 = to_dev(torch, pcm2)
        got2 = eng.stft_batch(dev2).cpu().numpy()
        ref2 = oracle.stream_process(pcm2, ch, Wt, Ht, threads=8)
        assert got2.shape == ref2.shape == (hops, 1, Wt - 1, 2) and mags_err(got2, ref2) <= 2.0
        assert np.array_equal(eng.stft_batch(dev2, first_frame=3, max_frames=777).cpu().numpy(), got2[3:780])
    if variant == "tuned" and not paired and ch in (8, 2):
        # the sliding window against the instantiation that requests every sample: hop position t at hop 512 IS hop position 2 t at hop 256 --
        # the same arithmetic in the same order, so the same bytes (3 001 hop positions: runs of 47 / 12 transforms per workgroup)
        hops = 3001
        dev4 = to_dev(torch, oracle.white_noise((Wt + (hops - 1) * Ht) * ch, seed=123 + ch))
        slid = eng.stft_batch(dev4)
        half = engine(window_samples=Wt, hop_samples=Ht // 2, channels=ch)
        every = half.stft_batch(dev4)
        assert every.shape[0] == 2 * hops - 1 and torch.equal(slid, every[::2])
        half.close()
        del slid, every, dev4
    if variant == "tuned" and not paired:
        # any other hop: every transform requests its own 16 samples per thread (the instantiation without the sliding window)
        for hop in (256, 1024, 500):
            other = engine(window_samples=Wt, hop_samples=hop, channels=ch)
            assert other.info.stft_kernel == 10
            hops = 37
            pcm3 = oracle.white_noise((Wt + (hops - 1) * hop) * ch, seed=5 + hop)
            got3 = other.stft_batch(to_dev(torch, pcm3)).cpu().numpy()
            ref3 = oracle.stream_process(pcm3, ch, Wt, hop, threads=8)
            assert got3.shape == ref3.shape and mags_err(got3, ref3) <= 2.0
            other.close()
    # the pixel path rides on it through the two-kernel route
    eng.set_builtin_gradient("viridis")
    rg = eng.render_batch(dev).cpu().numpy()
    own = oracle.render_columns(got.reshape(-1, Wt - 1, 2), SR, np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz"))["viridis"])
    assert np.array_equal(rg.reshape(own.shape), own)


@pytest.mark.parametrize("Wt,Ht", [(512, 64), (256, 100), (1024, 333), (4096, 512), (2400, 93), (735, 200), (1102, 100)])
def test_generic_kernel_pairs_mono_frames_by_global_index(torch_cuda, mags_err, Wt, Ht):
    # sizes served by the generic power-of-two kernel (W < 512), the mixed-radix kernel (4800 = 2^6 3 5^2, 1470 = 2 3 5 7^2,
    # and the powers of two from W = 512 on that have no tuned kernel: 1024 = 4 x 16 x 16, 2048 = 8 x 16 x 16, 8192 = 4 x 8 x 16 x 16) and the
    # chirp-z kernel (2204 = 4 * 19 * 29): a mono stream rides two frames per transform there too
    # (frames 2q and 2q+1 in the real / imaginary part), any sub-range writes the bytes of the full run, and
    # the default (no flag) is the reference's (s, s) dataflow
    torch = torch_cuda
    pcm = oracle.white_noise(Wt + 37 * Ht + 5, seed=Wt)
    dev = to_dev(torch, pcm)
    ref = oracle.stream_process(pcm, 1, Wt, Ht, threads=8)
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=1, paired_frames=True)
    assert eng.info.stft_kernel == ((0 if Wt < 512 else 6) if Wt & (Wt - 1) == 0 else (4 if Wt == 1102 else (9 if Wt == 2400 else 6)))
    tol = 2.0
    got = eng.stft_batch(dev).cpu().numpy()
    assert got.shape == ref.shape == (38, 1, Wt - 1, 2)
    assert mags_err(got, ref) <= tol and np.array_equal(got[..., 0], got[..., 1])
    for first, count in [(1, 36), (7, 1), (36, 2), (0, 37), (5, 6)]:
        assert np.array_equal(eng.stft_batch(dev, first_frame=first, max_frames=count).cpu().numpy(), got[first:first + count])
    ind_eng = engine(window_samples=Wt, hop_samples=Ht, channels=1)            # the default: every frame its own (s, s) transform
    ind = ind_eng.stft_batch(dev).cpu().numpy()
    assert mags_err(ind, ref) <= tol and mags_err(ind, got.astype(np.float64)) <= tol
    for first, count in [(1, 36), (7, 1), (5, 6)]:
        assert np.array_equal(ind_eng.stft_batch(dev, first_frame=first, max_frames=count).cpu().numpy(), ind[first:first + count])


def test_short_ragged_and_empty_inputs(torch_cuda):
    torch = torch_cuda
    eng = engine(window_samples=W, hop_samples=H, channels=2)
    assert eng.num_frames(0) == 0 and eng.num_frames(W - 1) == 0 and eng.num_frames(W) == 1
    short = torch.zeros(2 * (W - 1), device="cuda")
    assert eng.stft_batch(short).shape == (0, 1, M, 2)           # None -> no frames, no error
    assert eng.render_batch(short).shape == (0, 1, R, 4)
    assert eng.process_one(np.zeros((W - 1, 2), np.float32)) is None
    ragged = to_dev(torch, oracle.white_noise(2 * (W + H + 100)))  # 100 trailing samples unused
    assert eng.stft_batch(ragged).shape[0] == 2
    # first_frame / max_frames window
    pcm = oracle.white_noise(2 * (W + 7 * H), seed=2)
    full = eng.stft_batch(to_dev(torch, pcm)).cpu().numpy()
    part = eng.stft_batch(to_dev(torch, pcm), first_frame=3, max_frames=2).cpu().numpy()
    assert np.array_equal(part, full[3:5])
    assert eng.stft_batch(to_dev(torch, pcm), first_frame=99).shape[0] == 0
    # mono: two frames share a transform, paired by GLOBAL index -- any sub-range gives the same bytes
    for kw in (dict(), dict(paired_frames=True)):
        mono = engine(window_samples=W, hop_samples=H, channels=1, **kw)
        m = to_dev(torch, oracle.white_noise(W + 12 * H, seed=6))
        full = mono.stft_batch(m)
        for first, cnt in ((1, 5), (3, 2), (4, 9), (12, 1), (7, 100)):
            assert torch.equal(mono.stft_batch(m, first_frame=first, max_frames=cnt), full[first:first + cnt])
        assert torch.equal(mono.render_batch(m, first_frame=5, max_frames=4), mono.render_batch(m)[5:9])


def test_process_one_mirrors_process(torch_cuda, mags_err):
    from spectrogram_rs_amd import FastFourierTransform
    fft = FastFourierTransform(48000.0, 2048 / 48000.0 + 1e-7)
    assert fft.num_input_samples() == W and fft.num_output_frequencies() == M and fft.sample_rate() == 48000.0
    lr = oracle.white_noise(2 * W, seed=9).reshape(-1, 2)
    out = fft.process(lr)
    assert out.shape == (M, 2) and mags_err(out, oracle.np_truth_frame(lr, W)) <= 1.0
    assert fft.process(lr[:-1]) is None                       # fft.rs:72
    assert fft.process(iter([tuple(x) for x in lr])) is not None  # any iterable of (l, r)


@pytest.mark.parametrize("route", es.ROUTES, ids=lambda r: r.name)
def test_process_one_on_every_route(torch_cuda, mags_err, route):
    """sgx_process_one is the one caller whose channel count (2) is not the context's: one (l, r) frame on the context of every route,
    mono, four- and eight-channel ones included, against the float64 truth at the row's own floor."""
    eng = engine(**route.engine_kwargs())
    assert eng.info.stft_kernel == route.kernel
    Wt = route.W
    lr = oracle.white_noise(2 * Wt, seed=0x0E + Wt).reshape(-1, 2)
    out = eng.process_one(lr)
    assert out is not None and out.shape == (Wt - 1, 2)
    err = mags_err(out, es.truth_frame(lr, Wt), route.floor)
    print(f"{route.name}: {err:.4f}")
    assert err <= 1.0
    assert eng.process_one(lr[:-1]) is None                   # W - 1 pairs: None (fft.rs:72)


def test_unsupported_length_is_reported_not_approximated(torch_cuda):
    from spectrogram_rs_amd import SgxError
    with pytest.raises(SgxError) as ei:
        engine(window_samples=6001)  # 2W = 12002 = 2 * 17 * 353: not 7-smooth, and 3W - 1 > 16384 rules the chirp-z kernel out
    assert ei.value.code == -2 and "12002" in str(ei.value)
    with pytest.raises(SgxError):
        engine(window_samples=16384)  # 2W = 32768 does not fit the LDS
    assert engine(window_samples=5000).info.stft_kernel == 6    # 10000 = 2^4 5^4: mixed radix
    assert engine(window_samples=6000).info.stft_kernel == 6    # 12000 = 2^5 3 5^3: past the chirp-z range, still served
    assert engine(window_samples=10240).info.stft_kernel == 6   # 20480 = 2^12 5: the largest transform one CU's LDS holds
    with pytest.raises(SgxError):
        engine(window_samples=10290)                            # 20580 = 2^2 3 5 7^3: smooth but 164 640 B
    assert engine(window_samples=5003).info.stft_kernel == 4    # 10006 = 2 * 5003: chirp-z


@pytest.mark.parametrize("chirp_z", [False, True])
@pytest.mark.parametrize("sr,period,Wexp", [(48000.0, 0.05, 2400), (44100.0, 0.05, 2205), (48000.0, 0.01, 480), (8000.0, 0.0125, 100),
                                            (22050.0, 0.05, 1102), (48000.0, 0.0386, 1852), (192000.0, 0.05, 9600)])
def test_duration_sized_windows_like_the_app(torch_cuda, mags_err, sr, period, Wexp, chirp_z):
    # FastFourierTransform::new(sample_rate, 0.05) (gpu_spectrogram.rs:323): W = 2400 / 2205, 2W not a power of two.
    # Lengths with prime factors 2, 3, 5, 7 only (4800, 4410, 960, 200; 19 200 at 192 kHz) take the mixed-radix kernel, the others
    # (2204 = 4 * 19 * 29, 3704 = 8 * 463) the chirp-z kernel, which force_generic selects for the smooth ones too.
    torch = torch_cuda
    from spectrogram_rs_amd import SpectrogramEngine
    if Wexp == 9600 and chirp_z:
        pytest.skip("2W = 19 200 is beyond the chirp-z kernel (3W - 1 > 16384): mixed radix only")
    eng = SpectrogramEngine(sr, period=period, stride=2.0 / 1024, channels=2, force_generic=chirp_z)
    smooth = Wexp in (2400, 2205, 480, 100, 9600)
    assert eng.W == Wexp == oracle.window_samples(sr, period) and eng.info.stft_kernel == ((9 if Wexp == 2400 else 6) if smooth and not chirp_z else 4)
    Ht = eng.H
    assert Ht == oracle.hop_samples(sr, 2.0 / 1024)
    n = Wexp + 12 * Ht + 5
    pcm = oracle.white_noise(2 * n, seed=13)
    got = eng.stft_batch(to_dev(torch, pcm)).cpu().numpy()
    ref = oracle.stream_process(pcm, 2, Wexp, Ht, threads=8)
    assert got.shape == ref.shape == (13, 1, Wexp - 1, 2)
    truth = np.stack([oracle.np_truth_frame(pcm.reshape(-1, 2)[t * Ht:t * Ht + Wexp], Wexp) for t in (0, 7, 12)])
    # every kernel, the chirp-z one (two FFTs + three chirp products in float32) included, is held to 1x the tolerance
    # against the float64 truth and 2x against the float32 oracle (two float32 transforms)
    assert mags_err(got[[0, 7, 12], 0], truth) <= 1.0
    if eng.info.stft_kernel in (6, 9) or max(oracle_prime_factor(2 * Wexp), 2) <= 64:
        assert mags_err(got, ref) <= 2.0   # (a large prime factor is an O(p^2) float32 sum in the float32 oracle: no reference)
    # the pixel path rides on it (two-kernel route) and is bit-exact on the engine's own magnitudes
    eng.set_builtin_gradient("viridis")
    rgba = eng.render_batch(to_dev(torch, pcm)).cpu().numpy()
    own = oracle.render_columns(got[:, 0], int(sr), np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz"))["viridis"])
    assert np.array_equal(rgba[:, 0], own)


def test_stream_wrapper_on_gpu(torch_cuda, mags_err):
    from spectrogram_rs_amd import AudioStreamTransform, FastFourierTransform, RingBuffer
    rb = RingBuffer(1 << 16)
    lr = oracle.white_noise(2 * (W + 5 * 93 + 40), seed=4).reshape(-1, 2)
    rb.push_iter(lr)
    st = AudioStreamTransform(rb, FastFourierTransform(48000.0, 2048 / 48000.0 + 1e-7), 2.0 / 1024)
    frames = list(st.process())
    assert st.stride_samples() == 93 and len(frames) == 6
    ref = oracle.stream_process(lr, 2, W, 93)
    assert mags_err(np.stack(frames), ref[:, 0]) <= 2.0
    assert len(rb) == len(lr) - 7 * 93


@pytest.mark.parametrize("Wt", [2048, 2400, 8192, 1102])
def test_hann_table_is_the_oracles_bit_for_bit(torch_cuda, Wt):
    # quirk Q6 (fft.rs:61) is a statement about bits: 0.5 * (1 - cosf((TAU_f32 * i as f32) / W as f32)), every operation in
    # float32 in that order.  The table the kernels multiply by is the oracle's, bit for bit -- and so is what they apply:
    # a unit impulse in the left channel at sample i comes out as 2 hann[i] / W in every bin of the left magnitude
    eng = engine(window_samples=Wt, hop_samples=max(Wt // 8, 1), channels=2)
    win = eng.window()
    ref = oracle.hann_window(Wt)
    assert win.dtype == ref.dtype == np.float32 and np.array_equal(win.view(np.uint32), ref.view(np.uint32))
    assert win[0] == 0.0 and abs(float(win[Wt // 2]) - 1.0) < 1e-6          # periodic Hann: denominator W, not W - 1
    torch = torch_cuda
    for i in (1, Wt // 3, Wt - 1):
        lr = np.zeros((Wt, 2), np.float32)
        lr[i, 0] = 1.0
        got = eng.stft_batch(to_dev(torch, lr)).cpu().numpy()[0, 0]
        expect = 2.0 * np.float64(ref[i]) / Wt   # |L^[k]| = hann[i] for every k, scaled by 2 / W (fft.rs:92-98)
        assert np.abs(got[:, 0] - expect).max() <= 4e-7 * max(expect, 1e-30) + 1e-12 and np.abs(got[:, 1]).max() <= 4e-7 * expect + 1e-12


def _error_bands(got, truth):
    peak = np.abs(truth).max(axis=(1, 2), keepdims=True)
    level = 20 * np.log10(np.maximum(np.abs(truth), 1e-300) / peak)
    rel = np.abs(got - truth) / np.maximum(np.abs(truth), 1e-300)
    ab = np.abs(got - truth) / peak
    rows = []
    for lo in range(0, 160, 10):
        m = (level <= -lo) & (level > -(lo + 10))
        if m.any():
            rows.append((lo, int(m.sum()), float(rel[m].max()), float(ab[m].max())))
    return rows


@pytest.mark.parametrize("name,Wt,Ht,ch,kw", [("4096 mono, real-input", 2048, 256, 1, {}), ("4096 mono pairs", 2048, 256, 1, {"paired_frames": True}),
                                              ("4096 stereo", 2048, 256, 2, {}),
                                              ("16384 stereo", 8192, 512, 2, {}), ("4800 mixed radix", 2400, 93, 2, {}),
                                              ("2204 chirp-z", 1102, 100, 2, {}), ("3704 chirp-z", 1852, 100, 2, {}),
                                              ("2048 generic", 1024, 128, 2, {})])
def test_error_by_level_against_float64_truth(torch_cuda, name, Wt, Ht, ch, kw):
    # What "1e-5 relative" can and cannot mean for a float32 transform, measured instead of assumed: per 10 dB band below
    # the frame peak, the worst PURE relative error and the worst absolute error (as a fraction of the frame peak) of the
    # GPU magnitudes against numpy's float64 FFT of the reference's f32-windowed frame.  Asserted: 1e-5 relative in every
    # band down to 30 dB below the peak, 3e-7 of the peak everywhere (the floor of tests/conftest.py is 2e-7 from -34 dB).
    torch = torch_cuda
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=ch, **kw)
    frames = 8 if Wt >= 8192 else 16
    n = (frames - 1) * Ht + Wt
    t = np.arange(n, dtype=np.float64) / 48000.0
    tone = (0.5 * np.sin(2 * np.pi * 997.0 * t)).astype(np.float32) + (1e-4 * oracle.white_noise(n, seed=3)).astype(np.float32)
    sigs = {"white noise": oracle.white_noise(n * ch, seed=77),
            "tone + noise 74 dB down": np.repeat(tone, ch) if ch > 1 else tone,
            "sweep": np.repeat(oracle.sine_sweep(n), ch) if ch > 1 else oracle.sine_sweep(n)}
    print(f"\n{name}: kernel {eng.info.stft_kernel}")
    for sname, pcm in sigs.items():
        got = eng.stft_batch(to_dev(torch, pcm)).cpu().numpy().astype(np.float64)[:, 0]
        lr = pcm.reshape(-1, ch) if ch > 1 else np.stack([pcm, pcm], 1)
        truth = np.stack([oracle.np_truth_frame(lr[f * Ht:f * Ht + Wt, :2], Wt) for f in range(got.shape[0])])
        for lo, cnt, rel, ab in _error_bands(got, truth):
            print(f"  {sname:24s} {-lo:5d}..{-lo - 10:5d} dB  bins {cnt:7d}  worst rel {rel:8.2e}  worst abs/peak {ab:8.2e}")
            assert ab <= 3e-7, (name, sname, lo, ab)
            if lo < 30:
                assert rel <= 1e-5, (name, sname, lo, rel)


# ---- properties at sizes the oracle does not reach -----------------------------------------------

def test_full_size_properties(torch_cuda, mags_err):
    # BASELINE config 2 at its own size: 1e6 frames (256 001 792 samples in, 16.4 GB out)
    torch = torch_cuda
    F = 1_000_000
    eng = engine(window_samples=W, hop_samples=H, channels=1)
    n = (F - 1) * H + W
    pcm = eng.white_noise(n)
    assert np.array_equal(pcm[:4096].cpu().numpy(), oracle.white_noise(4096))      # generator parity
    assert np.array_equal(pcm[n - 512:].cpu().numpy(), oracle.white_noise(512, first=n - 512))
    mags = eng.stft_batch(pcm)
    assert mags.shape == (F, 1, M, 2) and bool(torch.isfinite(mags).all())
    # 1 024 sampled frames against the oracle, t = i*977 mod F
    ts = [(i * 977) % F for i in range(1024)]
    host = pcm.cpu().numpy()
    ref = np.stack([oracle.fft_process(np.stack([host[t * H:t * H + W]] * 2, 1), W) for t in ts])
    got = mags[ts, 0].cpu().numpy()
    assert mags_err(got, ref) <= 2.0
    # north_star's own bound at the full size: 1 x against the float64 truth of the reference's f32-windowed frame (fft.rs:81-98)
    truth = np.stack([oracle.np_truth_frame(np.stack([host[t * H:t * H + W]] * 2, 1), W) for t in ts])
    assert mags_err(got, truth) <= 1.0
    # homogeneity: halving the input (exact in f32) halves every magnitude bit for bit
    half = eng.stft_batch(pcm * 0.5)
    half *= 2.0
    assert bool(torch.equal(half, mags))
    del half
    # the first transform of a workgroup's run is a transform like any other: a shorter launch that starts one frame on has ~1000 run
    # starts of its own, every one of them the middle of a run of the full launch -- same bytes (this is what catches state a kernel
    # carries into its loop: registers, LDS, M0)
    shifted = eng.stft_batch(pcm, first_frame=1, max_frames=200_000)
    assert bool(torch.equal(shifted, mags[1:200_001]))
    del shifted
    # Parseval per frame: sum_k (m_k W/2)^2 over k=1..W-1 vs the windowed energy (DC/Nyquist excluded: loose bound)
    win = torch.from_numpy(eng.window()).cuda()
    idx = torch.arange(W, device="cuda")[None, :] + (torch.tensor(ts, device="cuda") * H)[:, None]
    e_time = ((pcm[idx] * win) ** 2).sum(1) * W  # = (1/2) sum over all P bins |F|^2 = P/2 * energy
    e_freq = ((mags[ts, 0, :, 0].double() * (W / 2.0)) ** 2).sum(1)
    rel = ((e_freq - e_time.double()).abs() / e_time.double()).max().item()
    assert rel < 2e-2
    # determinism and shard-independence: any split of the frame range gives the same bytes
    a = eng.checksum(mags)
    del mags
    again = eng.stft_batch(pcm)
    assert eng.checksum(again) == a
    del again
    lo = eng.stft_batch(pcm, first_frame=0, max_frames=F // 2)
    words_lo, c_lo = lo.numel(), eng.checksum(lo)
    del lo
    hi = eng.stft_batch(pcm, first_frame=F // 2)
    assert (c_lo + eng.checksum(hi, base_word=words_lo)) % (1 << 64) == a


def test_full_size_stereo_properties(torch_cuda, mags_err):
    # the (l, r) stream the reference actually feeds (audio_input_list_model.rs:70-72) at BASELINE config 2's size: 1e6 frames through the
    # 4096-point kernel's sliding-window instantiation (every workgroup a run of ~977 transforms)
    torch = torch_cuda
    F = 1_000_000
    eng = engine(window_samples=W, hop_samples=H, channels=2)
    assert eng.info.stft_kernel == 2
    n = (F - 1) * H + W
    pcm = eng.white_noise(n)
    assert pcm.numel() == 2 * n
    mags = eng.stft_batch(pcm)
    assert mags.shape == (F, 1, M, 2) and bool(torch.isfinite(mags).all())
    # 512 sampled frames against the oracle: t = i * 977 mod F, first and last included
    ts = sorted(set([(i * 977) % F for i in range(510)] + [0, F - 1]))
    host_idx = (torch.arange(W, device="cuda")[None, :] + (torch.tensor(ts, device="cuda") * H)[:, None])
    lr = pcm.view(-1, 2)[host_idx].cpu().numpy()                                  # [frames][W][2]
    ref = np.stack([oracle.fft_process(f, W) for f in lr])
    got = mags[ts, 0].cpu().numpy()
    assert mags_err(got, ref) <= 2.0
    assert mags_err(got, np.stack([oracle.np_truth_frame(f, W) for f in lr])) <= 1.0      # north_star's bound, 1 x, at the full size
    # left / right separation at full size: silencing the right channel leaves the left column bit for bit where the right was
    # already zero -- checked the cheap way round: a stream with r = 0 gives right magnitudes of exactly zero in every frame
    only_l = pcm.clone().view(-1, 2)
    only_l[:, 1] = 0.0
    ml = eng.stft_batch(only_l.view(-1))
    assert bool((ml[..., 0] >= 0).all()) and float(ml[..., 1].abs().max()) <= 1e-6 * float(ml[..., 0].max())
    del ml, only_l
    # homogeneity (exact in float32) and shard independence
    half = eng.stft_batch(pcm * 0.5)
    half *= 2.0
    assert bool(torch.equal(half, mags))
    del half
    # run starts of a shorter, shifted launch against the middle of the full launch's runs (see test_full_size_properties)
    shifted = eng.stft_batch(pcm, first_frame=1, max_frames=200_000)
    assert bool(torch.equal(shifted, mags[1:200_001]))
    del shifted
    a = eng.checksum(mags)
    del mags
    lo = eng.stft_batch(pcm, first_frame=0, max_frames=333_333)
    words_lo, c_lo = lo.numel(), eng.checksum(lo)
    del lo
    hi = eng.stft_batch(pcm, first_frame=333_333)
    assert (c_lo + eng.checksum(hi, base_word=words_lo)) % (1 << 64) == a


def test_full_size_config4_properties(torch_cuda, mags_err):
    # BASELINE config 4 at its own size: W 8192 / P 16384, hop 512, 8 interleaved channels, 1e5 hop positions =
    # 4e5 transforms, 1.64 GB in, 26.2 GB out -- output offsets far past 2^32 bytes (row 16 385 of the output starts there).
    torch = torch_cuda
    Wt, Ht, ch, hops = 8192, 512, 8, 100_000
    Mt = Wt - 1
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=ch)
    assert eng.info.stft_kernel == 10, "the tuned 16384-point kernel must be the one that runs"
    n = (hops - 1) * Ht + Wt
    pcm = eng.white_noise(n)
    assert pcm.numel() == n * ch
    mags = eng.stft_batch(pcm)
    assert mags.shape == (hops, ch // 2, Mt, 2) and mags.numel() * 4 == 26_211_200_000
    for lo in range(0, hops, 10_000):                   # finite everywhere (in pieces: isfinite materialises a byte per element)
        assert bool(torch.isfinite(mags[lo:lo + 10_000]).all())
    # 256 sampled (hop, pair) rows against the oracle: hop = i * 977 * 41 mod 1e5 (spread over the whole range, first and last
    # included), pair = i mod 4 -- every row at 1 x the tolerance of the float64 truth and 2 x the float32 oracle
    picks = [((i * 977 * 41) % hops, i % 4) for i in range(254)] + [(0, 0), (hops - 1, 3)]
    assert max(h for h, _ in picks) * 4 * Mt * 8 > 1 << 34          # rows far past the 4 GiB and 16 GiB byte offsets
    pcm2d = pcm.view(n, ch)
    got = np.stack([mags[h, pr].cpu().numpy() for h, pr in picks])
    host = [pcm2d[h * Ht:h * Ht + Wt, 2 * pr:2 * pr + 2].cpu().numpy() for h, pr in picks]
    # generator parity at the far end of the stream: channel c is the mono generator seeded seed + c
    tail = pcm2d[n - 256:].cpu().numpy()
    for c_ in (0, 3, 7):
        assert np.array_equal(tail[:, c_], oracle.white_noise(256, first=n - 256, seed=0x5EED0001 + c_))
    ref32 = np.stack([oracle.fft_process(x, Wt) for x in host])
    ref64 = np.stack([oracle.np_truth_frame(x, Wt) for x in host])
    assert mags_err(got, ref64, FLOOR_K16) <= 1.0
    assert mags_err(got, ref32, FLOOR_K16) <= 2.0
    # determinism: the same bytes again (the 16-byte store hazard of round 3 showed as a few wrong words per launch, now and then)
    a = eng.checksum(mags)
    del mags
    again = eng.stft_batch(pcm)
    assert eng.checksum(again) == a
    del again
    # shard independence across an ODD split (33 333 / 66 667 hop positions: mid-XCD-eighth, mid-pair-group): the two ranges,
    # computed by separate calls, checksum to the full run's value
    cut = 33_333
    lo = eng.stft_batch(pcm, first_frame=0, max_frames=cut)
    words_lo, c_lo = lo.numel(), eng.checksum(lo)
    del lo
    hi = eng.stft_batch(pcm, first_frame=cut)
    assert hi.shape[0] == hops - cut
    assert (c_lo + eng.checksum(hi, base_word=words_lo)) % (1 << 64) == a


@pytest.mark.parametrize("interp", [1, 0])
def test_full_size_pixel_properties(torch_cuda, gradients, interp):
    # BASELINE config 3 at its own size: 1e6 frames of the same stream -> 1024 log rows -> Viridis RGBA (4.1 GB), fused kernel;
    # cosine (what BASELINE names) and cubic (what the reference runs)
    torch = torch_cuda
    F = 1_000_000
    eng = engine(window_samples=W, hop_samples=H, channels=1, interp=interp, gradient="viridis")
    assert eng.info.render_path & 1, "the fused PCM-to-pixel kernel must be the one that runs"
    pcm = eng.white_noise((F - 1) * H + W)
    px = eng.render_batch(pcm)
    assert px.shape == (F, 1, R, 4) and px.dtype == torch.uint8
    # 1 024 sampled columns, t = i*977 mod F: (a) stage-wise bit-exact -- the oracle's pixel stage over the magnitudes the
    # engine itself computes for those frames; (b) end to end against the oracle's own float32 transform: a pixel whose
    # level sits on a LUT boundary may move one step, nothing else may happen
    ts = [(i * 977) % F for i in range(1024)]
    got = px[ts, 0].cpu().numpy()
    host = pcm.cpu().numpy()
    own_mags = np.concatenate([eng.stft_batch(pcm, first_frame=t, max_frames=1).cpu().numpy()[:, 0] for t in ts[:128]])
    assert np.array_equal(got[:128], oracle.render_columns(own_mags, SR, gradients["viridis"], interp=interp))
    ref_mags = np.stack([oracle.fft_process(np.stack([host[t * H:t * H + W]] * 2, 1), W) for t in ts])
    ref = oracle.render_columns(ref_mags, SR, gradients["viridis"], interp=interp)
    lut = {tuple(c): i for i, c in enumerate(gradients["viridis"])}
    diff = np.argwhere((got != ref).any(axis=2))
    steps = [abs(lut[tuple(got[a, b, :3])] - lut[tuple(ref[a, b, :3])]) for a, b in diff]
    assert len(diff) <= 2e-3 * got.shape[0] * R and (not steps or max(steps) <= 1), (len(diff), max(steps or [0]))
    assert (got[..., 3] == 255).all()
    del host
    # run starts of a shorter, shifted launch against the middle of the full launch's runs (see test_full_size_properties)
    shifted = eng.render_batch(pcm, first_frame=1, max_frames=200_000)
    assert bool(torch.equal(shifted, px[1:200_001]))
    del shifted
    # determinism and shard-independence of the bytes
    a = eng.checksum(px)
    del px
    again = eng.render_batch(pcm)
    assert eng.checksum(again) == a
    del again
    lo = eng.render_batch(pcm, first_frame=0, max_frames=F // 2 + 1)    # an odd split: the boundary cuts a mono frame pair
    words_lo, c_lo = lo.numel() // 4, eng.checksum(lo)
    del lo
    hi = eng.render_batch(pcm, first_frame=F // 2 + 1)
    assert (c_lo + eng.checksum(hi, base_word=words_lo)) % (1 << 64) == a


def test_stream_longer_than_2_to_32_samples(torch_cuda, mags_err):
    # config 5 streams hold 25.6 G samples: every index on the path is 64-bit.  A 17 GB mono stream whose last
    # frames start beyond sample 2^32 (where the noise generator also mixes in the high word)
    torch = torch_cuda
    eng = engine(window_samples=W, hop_samples=H, channels=1, gradient="viridis")
    n = (1 << 32) + 70_000
    if torch.cuda.mem_get_info()[0] < 30 * (1 << 30):
        pytest.skip("needs 30 GB of free HBM")
    pcm = eng.white_noise(n)
    total = eng.num_frames(n)
    assert total == (n - W) // H + 1
    first = total - 6
    assert first * H > (1 << 32)
    got = eng.stft_batch(pcm, first_frame=first).cpu().numpy()
    rg = eng.render_batch(pcm, first_frame=first).cpu().numpy()
    del pcm
    host = oracle.white_noise(5 * H + W, first=first * H)
    assert not np.array_equal(host[:64], oracle.white_noise(64, first=first * H - (1 << 32)))  # not a 32-bit wrap
    ref = oracle.stream_process(host, 1, W, H)
    assert got.shape == ref.shape == (6, 1, M, 2) and mags_err(got, ref) <= 2.0
    own = oracle.render_columns(got[:, 0], SR, np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz"))["viridis"])
    assert np.array_equal(rg[:, 0], own)


def test_pixel_path_properties_at_scale(torch_cuda):
    # 131 072 frames through the fused kernel: equal to the two-kernel path on sampled columns, deterministic,
    # and independent of how the frame range is split (what rank sharding relies on)
    torch = torch_cuda
    F = 131_072
    fused = engine(window_samples=W, hop_samples=H, channels=1, interp=1, gradient="viridis")
    split = engine(window_samples=W, hop_samples=H, channels=1, interp=1, gradient="viridis", fused_render=False)
    pcm = fused.white_noise((F - 1) * H + W) * 0.1
    a = fused.render_batch(pcm)
    assert a.shape == (F, 1, R, 4) and int(a[..., 3].min()) == 255
    ck = fused.checksum(a)
    assert fused.checksum(fused.render_batch(pcm)) == ck
    for first, cnt in ((0, 3000), (50_001, 777), (F - 5, 5)):
        assert torch.equal(split.render_batch(pcm, first_frame=first, max_frames=cnt), a[first:first + cnt])
    parts = [fused.render_batch(pcm, first_frame=f0, max_frames=c) for f0, c in ((0, 40_000), (40_000, 50_001), (90_001, F - 90_001))]
    words = 0
    total = 0
    for t in parts:
        total = (total + fused.checksum(t, base_word=words)) % (1 << 64)
        words += t.numel() // 4
    assert total == ck


# ---- the pixel path --------------------------------------------------------------------------------

@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("grad", ["viridis", "magma"])
def test_render_stage_is_bit_exact_given_identical_magnitudes(torch_cuda, gradients, interp, grad):
    torch = torch_cuda
    eng = engine(window_samples=W, hop_samples=H, channels=1, interp=interp, gradient=grad)
    assert np.array_equal(eng.bin_edges(), oracle.bin_edges(R))
    pcm = oracle.white_noise(W + 15 * H, seed=21)
    mags = oracle.stream_process(pcm, 1, W, H)[:, 0]
    # widen the dynamic range so every LUT level and both clamps are exercised
    mags = (mags * np.logspace(-4, 1.5, mags.shape[0], dtype=np.float32)[:, None, None]).astype(np.float32)
    mags[3] = 0.0
    got = eng.render_mags(to_dev(torch, mags)).cpu().numpy()
    ref = oracle.render_columns(mags, SR, gradients[grad], interp=interp)
    assert got.shape == ref.shape == (16, R, 4)
    assert np.array_equal(got, ref)
    assert len(np.unique(ref[..., :3].reshape(-1, 3), axis=0)) > 200


@pytest.mark.parametrize("Wt,cols", [(2048, 700), (4096, 9), (512, 300)])
def test_render_stage_kernels_agree_with_the_oracle(torch_cuda, gradients, Wt, cols):
    # the standalone pixel stage has two kernels: the persistent two-pass one (column, samples and tables fit in
    # LDS; W <= 2048) and the general one (here W = 4096).  `cols` > workgroups in flight makes the persistent
    # workgroups walk several columns each.
    torch = torch_cuda
    eng = engine(window_samples=Wt, hop_samples=64, channels=2, gradient="magma")
    rng = np.random.default_rng(Wt)
    mags = (np.abs(rng.standard_normal((cols, Wt - 1, 2))) * np.logspace(-5, 0, cols)[:, None, None]).astype(np.float32)
    got = eng.render_mags(to_dev(torch, mags)).cpu().numpy()
    pick = np.unique(np.linspace(0, cols - 1, 12).astype(int))
    ref = oracle.render_columns(mags[pick], SR, gradients["magma"])
    assert got.shape == (cols, R, 4) and np.array_equal(got[pick], ref)
    # every column, against the same kernel run column by column (persistence must not leak state)
    one = np.stack([eng.render_mags(to_dev(torch, mags[i:i + 1])).cpu().numpy()[0] for i in (0, cols // 2, cols - 1)])
    assert np.array_equal(one, got[[0, cols // 2, cols - 1]])


def test_render_golden_columns(torch_cuda, gold):
    torch = torch_cuda
    g = gold("rgba_columns.npz")
    for name, interp in (("cubic", 0), ("cosine", 1)):
        eng = engine(window_samples=W, hop_samples=H, interp=interp, gradient="viridis")
        got = eng.render_mags(to_dev(torch, g["mags"])).cpu().numpy()
        assert np.array_equal(got, g["viridis_" + name])


def test_render_stereo_scheme_bit_exact(torch_cuda, gradients):
    torch = torch_cuda
    eng = engine(window_samples=W, hop_samples=H, channels=2)
    eng.set_gradient(gradients["plasma"], stereo=True)
    st = oracle.white_noise(2 * (W + 7 * H), seed=8).reshape(-1, 2) * np.array([1.0, 0.3], np.float32)
    mags = oracle.stream_process(st, 2, W, H)[:, 0]
    mags = (mags * np.logspace(-3, 1, 8, dtype=np.float32)[:, None, None]).astype(np.float32)
    mags[2] = 0.0  # l = r = 0 -> t = NaN -> index 0, alpha from silence
    got = eng.render_mags(to_dev(torch, mags)).cpu().numpy()
    ref = oracle.render_columns(mags, SR, gradients["plasma"], stereo=True)
    assert np.array_equal(got, ref)
    assert got[..., 3].min() == 0 and got[..., 3].max() == 255


@pytest.mark.parametrize("Wt,Ht,ch", [(1102, 100, 2), (551, 43, 2), (1102, 43, 1), (1852, 170, 2), (3001, 300, 1), (5461, 500, 2), (341, 30, 2), (345, 30, 4), (86, 11, 2), (171, 20, 1), (85, 10, 2)])
def test_chirp_z_through_the_composite_stages(torch_cuda, mags_err, Wt, Ht, ch):
    # lengths with a prime factor above 7 (1102 = 0.05 s at 22.05 kHz, 551 at 11.025 kHz): from W = 86 on the convolution's
    # power-of-two transforms run the composite-radix stages and their inverses (render_path bit 2); SGX_FLAG_FORCE_GENERIC
    # keeps the radix-4 ladder: both against the float64 truth, sub-ranges the same bytes, mono pairs by global index
    torch = torch_cuda
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=ch)
    lad = engine(window_samples=Wt, hop_samples=Ht, channels=ch, force_generic=True)
    assert eng.info.stft_kernel == lad.info.stft_kernel == 4
    assert bool(eng.info.render_path & 4) == (Wt >= 86) and not (lad.info.render_path & 4)
    n = Wt + 8 * Ht + 3
    pcm = oracle.white_noise(n * ch, seed=Wt)
    dev = to_dev(torch, pcm)
    got, old = eng.stft_batch(dev).cpu().numpy(), lad.stft_batch(dev).cpu().numpy()
    lr = pcm.reshape(-1, ch)
    for t in (0, 5, 8):
        truth = oracle.np_truth_frame(np.stack([lr[t * Ht:t * Ht + Wt, 0], lr[t * Ht:t * Ht + Wt, min(1, ch - 1)]], 1), Wt)
        assert mags_err(got[t, 0], truth, FLOOR_WIDE) <= 1.0 and mags_err(old[t, 0], truth, FLOOR_WIDE) <= 1.0
    assert got.shape == old.shape == (9, max(ch // 2, 1), Wt - 1, 2)
    for first, cnt in ((1, 4), (8, 1), (3, 5)):
        assert np.array_equal(eng.stft_batch(dev, first_frame=first, max_frames=cnt).cpu().numpy(), got[first:first + cnt])


@pytest.mark.parametrize("sr,Wexp,fixed", [(8000, 400, True), (16000, 800, True), (32000, 1600, True), (44100, 2205, True), (48000, 2400, True),
                                           (88200, 4410, True), (96000, 4800, True), (176400, 8820, True), (192000, 9600, True),
                                           (24000, 1200, True), (12000, 600, False), (64000, 3200, False)])
def test_duration_sized_windows_of_the_usual_sample_rates(torch_cuda, mags_err, sr, Wexp, fixed):
    # FastFourierTransform::new(sample_rate, 0.05) (gpu_spectrogram.rs:323): the lengths the usual device rates produce run
    # instantiations of the mixed-radix kernel whose plan is a compile-time constant (sgx_info.render_path bit 2), every
    # other smooth length the run-time geometry: same results either way, stereo and mono pairs, sub-ranges included
    torch = torch_cuda
    from spectrogram_rs_amd import SpectrogramEngine
    for ch in (2, 1):
        eng = SpectrogramEngine(float(sr), period=0.05, stride=0.004, channels=ch)
        assert eng.W == Wexp and eng.info.stft_kernel == (9 if Wexp == 2400 else 6) and bool(eng.info.render_path & 4) == fixed
        n = eng.W + 6 * eng.H + 5
        pcm = oracle.white_noise(n * ch, seed=sr % 1000)
        dev = to_dev(torch, pcm)
        got = eng.stft_batch(dev).cpu().numpy()
        ref = oracle.stream_process(pcm, ch, eng.W, eng.H, threads=8)
        assert got.shape == ref.shape and got.shape[0] == 7
        assert mags_err(got, ref) <= 2.0
        assert np.array_equal(eng.stft_batch(dev, first_frame=3, max_frames=3).cpu().numpy(), got[3:6])
        assert torch.equal(eng.stft_batch_f16(dev), torch.from_numpy(got).cuda().to(torch.float16))
        # PCM -> pixels: one kernel where the plan is compiled in and the column fits the transform's LDS image (render_path
        # bit 0), the same bytes as the pixel stage alone on the stored magnitudes and as the oracle on them
        eng.set_builtin_gradient("viridis")
        px = eng.render_batch(dev).cpu().numpy()
        assert np.array_equal(px, eng.render_mags(torch.from_numpy(got).cuda().reshape(-1, eng.M, 2)).cpu().numpy().reshape(px.shape))
        own = oracle.render_columns(got.reshape(-1, eng.M, 2), sr, np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz"))["viridis"])
        assert np.array_equal(px.reshape(own.shape), own)
        if sr in (44100, 48000, 88200, 96000):   # more bins than samples per column: the pixel stage fits the transform's image
            assert eng.info.render_path & 1
        split = SpectrogramEngine(float(sr), period=0.05, stride=0.004, channels=ch, fused_render=False)
        split.set_builtin_gradient("viridis")
        assert not (split.info.render_path & 1) and np.array_equal(split.render_batch(dev).cpu().numpy(), px)


@pytest.mark.parametrize("Wt,Ht,interp", [(1024, 128, "cubic"), (4096, 512, "cubic"), (4096, 512, "cosine"), (8192, 512, "cosine"), (300, 50, "cubic")])
def test_pixel_stage_alone_at_other_window_sizes(torch_cuda, gradients, Wt, Ht, interp):
    # sgx_render_mags picks its workgroup size by how many column images fit a CU's LDS (256 / 512 / 1024 threads at
    # 1023 / 4095 / 8191 bins) and keeps table entries in registers only in the first case: every shape against the oracle
    torch = torch_cuda
    code = {"cubic": oracle.INTERP_CUBIC, "cosine": oracle.INTERP_COSINE}[interp]
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=2, interp=code)
    eng.set_gradient(gradients["magma"])
    pcm = oracle.white_noise(2 * (Wt + 5 * Ht), seed=Wt)
    mags = eng.stft_batch(to_dev(torch, pcm))
    got = eng.render_mags(mags[:, 0]).cpu().numpy()
    ref = oracle.render_columns(mags[:, 0].cpu().numpy(), SR, gradients["magma"], interp=code)
    assert got.shape == ref.shape == (6, R, 4) and np.array_equal(got, ref)
    eng.set_gradient(gradients["plasma"], stereo=True)
    assert np.array_equal(eng.render_mags(mags[:, 0]).cpu().numpy(),
                          oracle.render_columns(mags[:, 0].cpu().numpy(), SR, gradients["plasma"], interp=code, stereo=True))


@pytest.mark.parametrize("scheme", ["lut256", "lut256_round", "brewer", "lut256_walk"])
def test_diverging_branch_at_its_switch_points(torch_cuda, gradients, scheme):
    # colorscheme.rs:63-66 on constant columns (the interpolators return a constant spectrum's value exactly): balances
    # that sit exactly on k / 256 and one float to either side, negative values (cubic overshoot), zeros, infinities
    # and NaN, levels across every alpha byte.  256-level palettes indexed floor(t n) take the division-free level and
    # the seeded alpha byte; round(t (n - 1)) and the ColorBrewer splines (segment search through the balance grid)
    # keep the double-precision quotient; SGX_FLAG_LUT_WALK keeps every search a bisection.
    torch = torch_cuda
    rng = np.random.default_rng(5)
    k = np.arange(1, 256, dtype=np.float32)
    l_tie, r_tie = k * np.float32(2.0 ** -10), (256 - k) * np.float32(2.0 ** -10)
    pairs = [np.stack([l_tie, r_tie], 1), np.stack([np.nextafter(l_tie, np.float32(0)), r_tie], 1),
             np.stack([np.nextafter(l_tie, np.float32(1)), r_tie], 1), np.stack([l_tie * np.float32(1e-3), r_tie * np.float32(1e-3)], 1)]
    mag = (10 ** rng.uniform(-6, 1, (3000, 2))).astype(np.float32) * rng.choice(np.array([1, 1, 1, -1], np.float32), (3000, 2))
    special = np.array([[0, 0], [0, 1e-3], [1e-3, 0], [np.inf, 1], [1, np.inf], [np.inf, np.inf], [np.nan, 1], [1, np.nan], [-1e-3, 1e-3],
                        [1e-3, -1e-3], [1e-20, 1e-20], [3e38, 3e38], [1e-45, 0], [-0.0, 0.0]], np.float32)
    lr = np.concatenate(pairs + [mag, special]).astype(np.float32)
    mags = np.repeat(lr[:, None, :], M, 1)
    kw = dict(window_samples=W, hop_samples=H, channels=2)
    dev = to_dev(torch, mags)
    if scheme == "brewer":
        # the oracle has no callback gradients: the all-bisection build of the same tables (SGX_FLAG_LUT_WALK: no balance
        # grid, no seeded alpha byte) is the check, and the oracle pins that build on a LUT in the other cases
        eng = engine(**kw)
        eng.set_builtin_scheme("spectral", stereo=True)
        walk = engine(lut_walk=True, **kw)
        walk.set_builtin_scheme("spectral", stereo=True)
        ref = walk.render_mags(dev).cpu().numpy()
    else:
        mode = oracle.LUT_ROUND_NM1 if scheme == "lut256_round" else oracle.LUT_FLOOR_N
        eng = engine(lut_index_mode=mode, lut_walk=(scheme == "lut256_walk"), **kw)
        eng.set_gradient(gradients["plasma"], stereo=True)
        ref = oracle.render_columns(mags, SR, gradients["plasma"], stereo=True, mode=mode)
    got = eng.render_mags(dev).cpu().numpy()
    assert np.array_equal(got, ref)


def test_threshold_tables_reproduce_log10_everywhere(torch_cuda, gradients):
    # dense sweep of powers across every LUT boundary: one bin per "column", constant spectrum
    torch = torch_cuda
    eng = engine(window_samples=W, hop_samples=H, gradient="viridis")
    rng = np.random.default_rng(0)
    p = np.concatenate([10 ** rng.uniform(-8, 0, 4000), [0.0, 1e-30, 1e-7, 0.1, 0.1000001, 1.0, 1e6]]).astype(np.float32)
    m = np.sqrt(p / 2).astype(np.float32)
    mags = np.repeat(m[:, None, None], M, 1).repeat(2, 2).astype(np.float32)
    got = eng.render_mags(to_dev(torch, mags)).cpu().numpy()
    ref = oracle.render_columns(mags, SR, gradients["viridis"])
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("paired", [False, True])
def test_fused_pcm_to_rgba_end_to_end(torch_cuda, gradients, paired):
    # end to end the magnitudes differ from the oracle's by float32 rounding, so a pixel that sits
    # on a LUT boundary may move by one step: report the rate, bound it, and bound the step.
    torch = torch_cuda
    for interp in (0, 1):
        eng = engine(window_samples=W, hop_samples=H, channels=1, interp=interp, gradient="viridis", paired_frames=paired)
        pcm = oracle.white_noise(W + 63 * H, seed=33) * np.float32(0.05)
        got = eng.render_batch(to_dev(torch, pcm)).cpu().numpy()[:, 0]
        mags = oracle.stream_process(pcm, 1, W, H)[:, 0]
        ref = oracle.render_columns(mags, SR, gradients["viridis"], interp=interp)
        assert got.shape == ref.shape == (64, R, 4)
        lut = {tuple(c): i for i, c in enumerate(gradients["viridis"])}
        gi = np.array([lut[tuple(c)] for c in got[..., :3].reshape(-1, 3)])
        ri = np.array([lut[tuple(c)] for c in ref[..., :3].reshape(-1, 3)])
        mismatch = (gi != ri).mean()
        assert mismatch < 2e-3 and np.abs(gi - ri).max() <= 1, (mismatch, np.abs(gi - ri).max())
        # and exactly equal to the render stage applied to the engine's own magnitudes
        own = eng.render_mags(eng.stft_batch(to_dev(torch, pcm))[:, 0].contiguous()).cpu().numpy()
        assert np.array_equal(got, own)


@pytest.mark.parametrize("channels,frames,mode", [(1, 37, {}), (1, 64, {}), (1, 37, {"paired_frames": True}), (1, 64, {"paired_frames": True}),
                                                  (1, 21, {"complex_mono": True}), (2, 21, {})])
@pytest.mark.parametrize("interp", [0, 1])
def test_fused_kernel_equals_two_kernel_path(torch_cuda, channels, frames, mode, interp):
    # the fused PCM -> RGBA kernel (magnitudes stay in LDS) must write the bytes of STFT + pixel stage -- in every mono mode (the
    # real-input kernel, frame pairs, (s, s) transforms) and for an (l, r) stream
    torch = torch_cuda
    n = W + (frames - 1) * H
    pcm = to_dev(torch, oracle.white_noise(n * channels, seed=77) * np.float32(0.1))
    fused = engine(window_samples=W, hop_samples=H, channels=channels, interp=interp, gradient="magma", **mode)
    split = engine(window_samples=W, hop_samples=H, channels=channels, interp=interp, gradient="magma", fused_render=False, **mode)
    a = fused.render_batch(pcm).cpu().numpy()
    b = split.render_batch(pcm).cpu().numpy()
    assert a.shape == (frames, 1, R, 4) and np.array_equal(a, b)
    # sub-ranges and odd counts (a mono transform carries two frames)
    c = fused.render_batch(pcm, first_frame=5, max_frames=7).cpu().numpy()
    assert np.array_equal(c, a[5:12])
    # the fused kernel's LUT index is its log2 seed plus ONE compare pair (the host has shown the seed is never off by
    # more than one -- also where the dB range starts below the 1e-7 power floor, min_db < -70); SGX_FLAG_LUT_WALK
    # makes it walk the thresholds from the seed instead, as it does where that proof fails -- the same bytes either
    # way, over the whole level range
    assert fused.info.render_path & 7 == 3 and split.info.render_path & 7 == 0
    kw = dict(window_samples=W, hop_samples=H, channels=channels, interp=interp, gradient="magma", **mode)
    walk = engine(lut_walk=True, **kw)
    low = engine(min_db=-110.0, max_db=-20.0, **kw)
    low_split = engine(min_db=-110.0, max_db=-20.0, fused_render=False, **kw)
    assert walk.info.render_path & 7 == 1 and low.info.render_path & 7 == 3
    for amp in (1.0, 1e-2, 1e-4, 0.0):       # every LUT index from the top of the ramp down to silence
        x = pcm * amp
        want = split.render_batch(x)
        assert torch.equal(fused.render_batch(x), want) and torch.equal(walk.render_batch(x), want)
        assert torch.equal(low.render_batch(x), low_split.render_batch(x))
    # a diverging scheme is not fused: still correct through the same entry point
    fused.set_gradient(np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz"))["plasma"], stereo=True)
    split.set_gradient(np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz"))["plasma"], stereo=True)
    assert np.array_equal(fused.render_batch(pcm).cpu().numpy(), split.render_batch(pcm).cpu().numpy())


@pytest.mark.parametrize("cfg", [
    dict(rows=1000, f_min=20.0, f_max=24000.0, min_db=-90.0, max_db=0.0, interp=0),      # rows not a multiple of 256, f_max at Nyquist
    dict(rows=7, f_min=100.0, f_max=8000.0, min_db=-60.0, max_db=-20.0, interp=1),        # fewer rows than threads
    dict(rows=2048, f_min=32.0, f_max=22030.0, min_db=-70.0, max_db=-10.0, interp=0, lut_index_mode=1),  # round-to-nearest LUT rule
    dict(rows=300, f_min=1.0, f_max=90000.0, min_db=-70.0, max_db=-10.0, interp=0),       # axis far outside the spectrum: index clamps at both ends
])
@pytest.mark.parametrize("channels", [1, 2])
def test_pixel_path_configuration_space(torch_cuda, gradients, cfg, channels):
    # fused kernel, two-kernel path and oracle agree for every axis / dB range / LUT rule (on the engine's own magnitudes); mono runs
    # the real-input kernel's pixel passes, (l, r) the complex kernel's.  rows = 7: the top rows average > 256 samples each -- fused
    # all the same (the row word holds 16 bits of count)
    torch = torch_cuda
    pcm = to_dev(torch, oracle.white_noise((W + 20 * H) * channels, seed=101) * np.float32(0.2))
    kw = dict(window_samples=W, hop_samples=H, channels=channels, gradient="inferno", **cfg)
    fused, split = engine(**kw), engine(fused_render=False, **kw)
    if cfg["rows"] == 7:
        assert fused.row_sample_counts().max() >= 256 and fused.info.render_path & 1, "the fused kernel must serve rows of 256 samples and more"
    a = fused.render_batch(pcm).cpu().numpy()[:, 0]
    b = split.render_batch(pcm).cpu().numpy()[:, 0]
    mags = fused.stft_batch(pcm).cpu().numpy()[:, 0]
    ref = oracle.render_columns(mags, SR, gradients["inferno"], R=cfg["rows"], f_min=cfg["f_min"], f_max=cfg["f_max"],
                                interp=cfg["interp"], min_db=cfg["min_db"], max_db=cfg["max_db"], mode=cfg.get("lut_index_mode", 0))
    assert a.shape == ref.shape == (21, cfg["rows"], 4)
    assert np.array_equal(a, b) and np.array_equal(a, ref)
    assert np.array_equal(fused.bin_edges(), oracle.bin_edges(cfg["rows"], cfg["f_min"], cfg["f_max"]))


@pytest.mark.parametrize("paired", [False, True])
def test_non_finite_and_extreme_samples(torch_cuda, gradients, paired):
    # NaN / inf / huge samples must not fault or poison neighbouring frames; colours follow Rust's
    # saturating casts (NaN -> index 0); frames without bad samples are unaffected
    torch = torch_cuda
    x = oracle.white_noise(W + 40 * H, seed=5) * np.float32(0.1)
    bad = x.copy()
    bad[W + 20 * H + 5] = np.nan          # touches frames 21..28 (every frame whose window covers it)
    bad[100] = np.float32(3e38)           # frame 0 only (sample 100 < H): overflows to inf in the FFT
    eng = engine(window_samples=W, hop_samples=H, channels=1, gradient="viridis", paired_frames=paired)
    assert bool(eng.info.render_path & 8) == (not paired)
    good_m = eng.stft_batch(to_dev(torch, x)).cpu().numpy()
    bad_m = eng.stft_batch(to_dev(torch, bad)).cpu().numpy()
    touched = np.zeros(41, bool)
    touched[0] = True
    n_idx = W + 20 * H + 5
    touched[[t for t in range(41) if t * H <= n_idx < t * H + W]] = True
    if paired:
        # SGX_FLAG_PAIRED_FRAMES: a transform carries frames 2j and 2j+1 (real / imaginary part): a non-finite sample also
        # reaches the partner frame of the same transform -- exactly as a non-finite LEFT sample reaches the
        # RIGHT channel of its frame in the reference's own (l + i r) packing (fft.rs:57,87-88)
        touched = touched | np.array([touched[min(t ^ 1, 40)] for t in range(41)])
    # default: every frame its own transform -- a bad sample reaches EXACTLY the frames whose window covers it (frame 1 shares a
    # workgroup iteration with frame 0, frame 20 with frame 21, frame 29 with frame 28: all three stay bit-identical)
    assert np.array_equal(bad_m[~touched], good_m[~touched])
    assert all(not np.isfinite(bad_m[t]).all() for t in np.flatnonzero(touched))
    if not paired:
        assert not touched[1] and not touched[20] and not touched[29] and touched[21] and touched[28]
    rg = eng.render_batch(to_dev(torch, bad)).cpu().numpy()[:, 0]
    ref = oracle.render_columns(bad_m[:, 0], SR, gradients["viridis"])
    assert np.array_equal(rg, ref)


SENTINEL_CASES = [
    # (window, hop, channels, flags): every kernel that holds two frames per workgroup iteration and drops the second of an odd launch
    (2048, 256, 1, {}),                          # K1R, sliding window
    (2048, 100, 1, {}),                          # K1R, any hop
    (2048, 256, 1, {"paired_frames": True}),     # K1, mono frame pairs
    (2048, 256, 2, {}),                          # K1, (l, r)
    (2400, 93, 1, {}),                           # mixed radix, real-input mode (two frames per workgroup to pixels)
    (2400, 93, 1, {"paired_frames": True}),      # K48 frame pairs
    (2205, 86, 1, {}),                           # mixed radix, odd window
    (1102, 43, 1, {}),                           # chirp-z, real-input mode
    (8192, 512, 1, {}),                          # K16 on a duplicated plane
]


@pytest.mark.parametrize("case", SENTINEL_CASES, ids=lambda c: "W%d-H%d-C%d%s" % (c[0], c[1], c[2], "-" + "-".join(c[3]) if c[3] else ""))
def test_rows_past_the_requested_count_are_never_written(torch_cuda, case):
    # an odd launch computes the absent second frame of its last pair and must drop it -- nothing may land in the caller's
    # buffer at or past row n.  The caller's buffer here is LARGER than the call needs, its tail filled with a sentinel; every output
    # kind (float rows, half rows, RGBA columns), odd and even counts, also behind a first_frame.
    torch = torch_cuda
    Wc, Hc, ch, kw = case
    eng = engine(window_samples=Wc, hop_samples=Hc, channels=ch, gradient="viridis", **kw)
    Mc = Wc - 1
    pcm = to_dev(torch, oracle.white_noise((Wc + 40 * Hc) * ch, seed=23) * np.float32(0.3))
    extra = 3
    for first, n in ((0, 1), (0, 5), (3, 7), (0, 8), (2, 33)):
        want_f = eng.stft_batch(pcm, first_frame=first, max_frames=n)
        buf = torch.full((n + extra, eng.pairs, Mc, 2), float("nan"), dtype=torch.float32, device="cuda")
        eng.stft_batch(pcm, first_frame=first, max_frames=n, out=buf)
        assert torch.equal(buf[:n], want_f) and bool(torch.isnan(buf[n:]).all()), ("f32 rows", first, n)
        want_h = eng.stft_batch_f16(pcm, first_frame=first, max_frames=n)
        bufh = torch.full((n + extra, eng.pairs, Mc, 2), float("nan"), dtype=torch.float16, device="cuda")
        eng.stft_batch_f16(pcm, first_frame=first, max_frames=n, out=bufh)
        assert torch.equal(bufh[:n], want_h) and bool(torch.isnan(bufh[n:]).all()), ("f16 rows", first, n)
        want_p = eng.render_batch(pcm, first_frame=first, max_frames=n)
        bufp = torch.full((n + extra, eng.pairs, R, 4), 0xA5, dtype=torch.uint8, device="cuda")
        eng.render_batch(pcm, first_frame=first, max_frames=n, out=bufp)
        assert torch.equal(bufp[:n], want_p) and bool((bufp[n:] == 0xA5).all()), ("rgba columns", first, n)
        # and in FRONT of the buffer: a call whose output starts inside a larger allocation leaves the rows before it alone
        big = torch.full((2 + n + extra, eng.pairs, Mc, 2), float("nan"), dtype=torch.float32, device="cuda")
        eng.stft_batch(pcm, first_frame=first, max_frames=n, out=big[2:])
        assert torch.equal(big[2:2 + n], want_f) and bool(torch.isnan(big[:2]).all()) and bool(torch.isnan(big[2 + n:]).all())


def test_frame_pairing_dynamic_range_and_independent_frames(torch_cuda, mags_err):
    # A mono transform carries two frames; float32 rounding of the louder one is the noise floor of the
    # quieter one (as left / right share one transform in the reference).  Frames that share 7/8 of their
    # samples are never far apart in level -- except across an isolated transient.  By default (W 2048 / H 256: the real-input
    # kernel) every frame gets its own transform, exactly the reference's dataflow;
    # paired_frames=True is the two-frames-per-transform mode.
    torch = torch_cuda
    x = oracle.white_noise(W + 3 * H, seed=9) * np.float32(1e-3)
    x[10] = 1.0                                  # a click inside frame 0 only (sample 10 < H)
    ref = np.stack([oracle.np_truth_frame(np.stack([x[t * H:t * H + W]] * 2, 1), W) for t in range(4)])
    paired = engine(window_samples=W, hop_samples=H, channels=1, paired_frames=True).stft_batch(to_dev(torch, x)).cpu().numpy()[:, 0]
    indep = engine(window_samples=W, hop_samples=H, channels=1).stft_batch(to_dev(torch, x)).cpu().numpy()[:, 0]   # the default at this window / hop
    cplx = engine(window_samples=W, hop_samples=H, channels=1, complex_mono=True).stft_batch(to_dev(torch, x)).cpu().numpy()[:, 0]
    assert mags_err(indep, ref) <= 1.0 and mags_err(cplx, ref) <= 1.0   # every frame within tolerance of the truth
    assert mags_err(paired[[0, 2, 3]], ref[[0, 2, 3]]) <= 1.0
    # frame 1 rides with the click: its error is bounded relative to the PAIR's peak, not its own
    pair_peak = np.abs(ref[:2]).max()
    assert np.abs(paired[1] - ref[1]).max() <= 1e-6 * pair_peak


@pytest.mark.parametrize("n_frames", [1, 2, 3, 64, 131, 2051])
def test_real_input_kernel_for_independent_mono_frames(torch_cuda, mags_err, n_frames):
    # A mono stream at W 2048 / H 256 (the headline's stream shape), DEFAULT flags: every frame is its own transform -- the
    # reference's (s, s) dataflow, audio_input_list_model.rs:67-69 + fft.rs:47-99 -- computed as a 2048-point complex transform of
    # the real frame + one butterfly per bin (csrc/stft4096_real.hip).  Against the float64 truth (1 x), the float32 oracle (2 x),
    # the literal (s, s) transform (SGX_FLAG_COMPLEX_MONO), the paired mode (pair-peak tolerance) and itself over sub-ranges,
    # odd counts and a misaligned stream.
    torch = torch_cuda
    n = W + (n_frames - 1) * H + 77
    pcm = oracle.white_noise(n, seed=1000 + n_frames)
    pcm[: min(n, 5000)] *= np.float32(0.01)                 # a level step inside the stream: frames of very different peaks
    dev = to_dev(torch, pcm)
    real = engine(window_samples=W, hop_samples=H, channels=1)
    cplx = engine(window_samples=W, hop_samples=H, channels=1, complex_mono=True)
    pair = engine(window_samples=W, hop_samples=H, channels=1, paired_frames=True)
    assert real.info.stft_kernel == 2 and real.info.render_path & 8 and not (cplx.info.render_path & 8) and not (pair.info.render_path & 8)
    got = real.stft_batch(dev).cpu().numpy()
    assert got.shape == (n_frames, 1, M, 2)
    pick = sorted(set(list(range(min(n_frames, 24))) + [n_frames - 1, n_frames // 2] + list(range(0, n_frames, 97))))
    truth = np.stack([oracle.np_truth_frame(np.stack([pcm[t * H:t * H + W]] * 2, 1), W) for t in pick])
    assert mags_err(got[pick, 0], truth) <= 1.0              # own-peak tolerance, every checked frame
    assert np.array_equal(got[..., 0], got[..., 1])          # (m, m): one spectrum, written twice
    ref32 = oracle.stream_process(pcm, 1, W, H, threads=8)
    assert mags_err(got, ref32) <= 2.0
    assert mags_err(got, cplx.stft_batch(dev).cpu().numpy().astype(np.float64)) <= 2.0
    assert _pair_error(pair.stft_batch(dev).cpu().numpy()[pick, 0], truth) <= 1.0 if pick == list(range(n_frames)) else True
    # frames are independent problems: any sub-range, from an odd first frame too, writes the bytes of the full run
    for first, cnt in ((0, 1), (1, 1), (1, 2), (2, 5), (n_frames - 1, 1), (n_frames // 2, n_frames)):
        if first >= n_frames:
            continue
        part = real.stft_batch(dev, first_frame=first, max_frames=cnt).cpu().numpy()
        assert np.array_equal(part, got[first:first + cnt]), (first, cnt)
    # half rows straight from the kernel = the float rows rounded to nearest even
    h = real.stft_batch_f16(dev)
    assert torch.equal(h, torch.from_numpy(got).cuda().to(torch.float16))
    assert torch.equal(real.stft_batch_f16(dev, first_frame=1, max_frames=3), h[1:4])
    # a stream that is 4- but not 8-byte aligned cannot be read as 8-byte columns: the (s, s) kernel takes it (own-peak tolerance)
    shifted = torch.empty(dev.numel() + 1, dtype=dev.dtype, device=dev.device)
    shifted[1:] = dev
    assert shifted[1:].data_ptr() % 8 == 4
    alt = engine(window_samples=W, hop_samples=H, channels=1, complex_mono=False).stft_batch(shifted[1:]).cpu().numpy()
    assert mags_err(alt[pick, 0], truth) <= 1.0
    assert np.array_equal(real.stft_batch(shifted[1:]).cpu().numpy(), alt)
    # determinism
    assert np.array_equal(real.stft_batch(dev).cpu().numpy(), got)


@pytest.mark.parametrize("Ht,off", [(2, 0), (100, 0), (128, 0), (512, 0), (1000, 0), (2048, 0), (3000, 0), (255, 0), (93, 0), (1, 0), (2047, 1), (256, 1),
                                    (256, 3), (100, 1)])
def test_real_input_kernel_at_other_hops(torch_cuda, mags_err, Ht, off):
    # W 2048 at ANY hop and any (4-byte) alignment of the stream: the default mono mode is the real-input kernel too (hops other than
    # 256: no sliding window, the eight columns of a frame pair are requested ahead of the stores).  An odd hop or a stream that starts
    # on an odd sample makes the 8-byte sample pairs 4-byte aligned: buffer loads of two dwords need dword alignment only.
    torch = torch_cuda
    frames = 37
    n = W + (frames - 1) * Ht + min(5, Ht - 1)        # a ragged tail shorter than one hop
    pcm = oracle.white_noise(n + off, seed=500 + Ht)
    pcm[(n + off) // 2:] *= np.float32(1e-3)
    dev = to_dev(torch, pcm)[off:]
    pcm = pcm[off:]
    eng = engine(window_samples=W, hop_samples=Ht, channels=1, interp=1, gradient="inferno")
    assert eng.info.render_path & 8
    got = eng.stft_batch(dev).cpu().numpy()
    truth = np.stack([oracle.np_truth_frame(np.stack([pcm[t * Ht:t * Ht + W]] * 2, 1), W) for t in range(frames)])
    assert got.shape == (frames, 1, M, 2)
    assert mags_err(got[:, 0], truth) <= 1.0                             # every frame, own peak
    cplx = engine(window_samples=W, hop_samples=Ht, channels=1, complex_mono=True).stft_batch(dev).cpu().numpy()
    assert mags_err(got, cplx.astype(np.float64)) <= 2.0
    pair = engine(window_samples=W, hop_samples=Ht, channels=1, paired_frames=True).stft_batch(dev).cpu().numpy()
    assert _pair_error(pair[:, 0], truth) <= 1.0                         # frame pairs (opt-in): the pair's peak
    for first, cnt in ((1, 1), (3, 6), (36, 1), (8, 100)):
        assert np.array_equal(eng.stft_batch(dev, first_frame=first, max_frames=cnt).cpu().numpy(), got[first:first + cnt])
    assert torch.equal(eng.stft_batch_f16(dev), torch.from_numpy(got).cuda().to(torch.float16))
    px = eng.render_batch(dev)
    assert torch.equal(px[:, 0], eng.render_mags(torch.from_numpy(got[:, 0]).cuda().contiguous()))
    assert torch.equal(eng.render_batch(dev, first_frame=5, max_frames=7), px[5:12])


@pytest.mark.parametrize("Wt,Ht,off", [(2400, 93, 0), (2400, 256, 1), (2205, 85, 0), (2205, 512, 0), (1200, 100, 0), (300, 7, 1), (4800, 1024, 0),
                                       (9600, 3000, 0), (1000, 250, 0), (1024, 256, 0), (4096, 512, 2), (441, 100, 0), (12, 2, 0), (9, 3, 0), (15, 4, 1), (512, 64, 0), (2000, 500, 0), (1944, 97, 0),
                                       (1102, 43, 0), (551, 100, 1), (3001, 300, 0), (171, 20, 0), (5461, 500, 0), (87, 9, 0), (1852, 170, 0)])
def test_real_input_mode_of_the_mixed_radix_kernel(torch_cuda, mags_err, Wt, Ht, off):
    # every window the mixed-radix kernel serves (2W = 2^a 3^b 5^c 7^d), a mono stream in the default mode: the W-point transform of
    # z[m] = x[2m] + i x[2m+1] and the untangling epilogue (stft_mixed.hip: untangle_store) -- compile-time plans (2400, 2205, 4800,
    # 9600 points ...) and the run-time plan, odd W (the last sample is half a pair), odd hops and a stream that is not 8-byte aligned
    # (scalar loads); W 2400 leaves the 4800-point kernel for it.  Against the float64 truth per frame, own peak.  The last seven: lengths
    # with a prime factor above 7 -- the chirp-z kernel (stft_kernel 4) in the same mode: a W-point chirp-z transform of ceil(W / 2) sample
    # pairs, a convolution of half the length, and the same untangling epilogue.
    torch = torch_cuda
    frames = 11
    n = Wt + (frames - 1) * Ht + min(3, Ht - 1)
    pcm = oracle.white_noise(n + off, seed=900 + Wt + Ht)
    pcm[(n + off) // 2:] *= np.float32(1e-3)
    dev = to_dev(torch, pcm)[off:]
    pcm = pcm[off:]
    Mt = Wt - 1
    eng = engine(window_samples=Wt, hop_samples=Ht, channels=1, interp=1, gradient="inferno")
    assert eng.info.stft_kernel in (4, 6, 9) and eng.info.render_path & 8
    got = eng.stft_batch(dev).cpu().numpy()
    truth = np.stack([oracle.np_truth_frame(np.stack([pcm[t * Ht:t * Ht + Wt]] * 2, 1), Wt) for t in range(frames)])
    assert got.shape == (frames, 1, Mt, 2)
    assert np.array_equal(got[..., 0], got[..., 1])
    assert mags_err(got[:, 0], truth, FLOOR_WIDE) <= 1.0
    cplx_eng = engine(window_samples=Wt, hop_samples=Ht, channels=1, complex_mono=True)
    assert not cplx_eng.info.render_path & 8
    cplx = cplx_eng.stft_batch(dev).cpu().numpy()
    assert mags_err(got, cplx.astype(np.float64), FLOOR_WIDE) <= 2.0                 # the same frames as (s, s) through the 2W-point plan
    for first, cnt in ((1, 1), (3, 6), (10, 1), (8, 100)):
        assert np.array_equal(eng.stft_batch(dev, first_frame=first, max_frames=cnt).cpu().numpy(), got[first:first + cnt])
    assert torch.equal(eng.stft_batch_f16(dev), torch.from_numpy(got).cuda().to(torch.float16))
    px = eng.render_batch(dev)
    assert torch.equal(px[:, 0], eng.render_mags(torch.from_numpy(got[:, 0]).cuda().contiguous()))
    assert torch.equal(eng.render_batch(dev, first_frame=5, max_frames=4), px[5:9])


def _pair_error(x, ref, first_frame=0):
    """mags_error with the PAIR's peak (frames 2j, 2j+1 by global index) in place of the frame's own: the tolerance a mono
    frame meets when it shares its transform with its neighbour, as left and right do in the reference (fft.rs:57,87-88)"""
    from conftest import PEAK_FLOOR, REL_TOL
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    own = np.abs(ref).max(axis=(-1, -2))
    pair = own.copy()
    for t in range(len(own)):
        q = (t + first_frame) ^ 1
        if 0 <= q - first_frame < len(own):
            pair[t] = max(own[t], own[q - first_frame])
    allow = np.maximum(REL_TOL * np.maximum(np.abs(ref), PEAK_FLOOR * pair[:, None, None]), 1e-30)
    return float((np.abs(x - ref) / allow).max())


@pytest.mark.parametrize("step_db", [20, 40, 60, None])
@pytest.mark.parametrize("kind", ["onset", "offset"])
def test_onsets_inside_one_hop_own_peak_tolerance_and_the_paired_bound(torch_cuda, mags_err, step_db, kind):
    # What two frames per transform cost in conformance, measured and bounded -- the mode of rounds 1-3's
    # headline, now SGX_FLAG_PAIRED_FRAMES at this window / hop and still the default at every other one.  A level step of
    # 20 / 40 / 60 dB -- or from digital silence (None) -- to full scale INSIDE ONE HOP, placed so that it falls between the two
    # frames of a pair: onset in [6H + W, 7H + W) is inside frame 7's last hop and outside frame 6; offset (loud -> quiet) at a
    # sample in [6H, 7H) leaves its last loud samples in frame 6's first hop and none in frame 7.  Also one step that does NOT
    # split a pair (between frames 9 and 10), where paired and independent modes must both hold the own-peak tolerance.
    #   every frame its own transform (the default here; the reference's (s, s) dataflow, audio_input_list_model.rs:67-69 + fft.rs:81-98):
    #       every frame within 1 x north_star's tolerance of the float64 truth against ITS OWN peak -- asserted;
    #   paired: every frame within 1 x the same tolerance against the PAIR's peak -- asserted; against its own peak
    #       the quiet frame of a split pair is off by up to the level ratio of the pair -- measured, printed, and bounded by
    #       that ratio (the statement "1e-7 of the pair's peak" of DESIGN section 4 as an assertion).
    torch = torch_cuda
    n = W + 15 * H
    quiet = np.float32(0.0 if step_db is None else 0.9 * 10.0 ** (-step_db / 20.0))
    loud = np.float32(0.9)
    noise = oracle.white_noise(n, seed=21)
    for cut, split_pair in ((6 * H + (W if kind == "onset" else 0) + 100, True), (10 * H + (W if kind == "onset" else 0) - 156, False)):
        gain = np.where(np.arange(n) < cut, quiet if kind == "onset" else loud, loud if kind == "onset" else quiet).astype(np.float32)
        x = noise * gain
        ref = np.stack([oracle.np_truth_frame(np.stack([x[t * H:t * H + W]] * 2, 1), W) for t in range(16)])
        own_peak = np.abs(ref).max(axis=(1, 2))
        indep = engine(window_samples=W, hop_samples=H, channels=1).stft_batch(to_dev(torch, x)).cpu().numpy()[:, 0]          # the default: every frame its own transform
        paired = engine(window_samples=W, hop_samples=H, channels=1, paired_frames=True).stft_batch(to_dev(torch, x)).cpu().numpy()[:, 0]
        assert mags_err(indep, ref) <= 1.0
        assert _pair_error(paired, ref) <= 1.0
        # sub-ranges pair by GLOBAL index: the same bound from an odd first frame
        part = engine(window_samples=W, hop_samples=H, channels=1, paired_frames=True).stft_batch(to_dev(torch, x), first_frame=5, max_frames=6).cpu().numpy()[:, 0]
        assert np.array_equal(part, paired[5:11])
        per_frame = np.array([mags_err(paired[t], ref[t]) for t in range(16)])
        worst = int(per_frame.argmax())
        ratio = np.array([max(own_peak[t], own_peak[t ^ 1]) / max(own_peak[t], 1e-30) for t in range(16)])
        print(f"  {kind} {step_db} dB, cut {cut} ({'splits a pair' if split_pair else 'between pairs'}): paired own-peak error "
              f"{per_frame.max():.3g} x tolerance at frame {worst} (pair level ratio {ratio[worst]:.3g}); independent {mags_err(indep, ref):.3g}")
        if step_db is not None:
            assert (per_frame <= np.maximum(1.0, ratio)).all()      # never worse than the pair's level ratio
        frames_far = [t for t in range(16) if ratio[t] < 1.5]
        assert mags_err(paired[frames_far], ref[frames_far]) <= 1.5   # frames whose partner is at their own level: (about) the own-peak tolerance


@pytest.mark.parametrize("kw", [dict(channels=1), dict(channels=1, paired_frames=True), dict(channels=2), dict(channels=1, force_generic=True),
                                dict(channels=2, window_samples=2400, hop_samples=93), dict(channels=1, window_samples=2400, hop_samples=93),
                                dict(channels=1, window_samples=2400, hop_samples=93, paired_frames=True), dict(channels=1, window_samples=1024, hop_samples=100, paired_frames=True),
                                dict(channels=2, window_samples=2205, hop_samples=86), dict(channels=4, window_samples=1600, hop_samples=50),
                                dict(channels=2, window_samples=1102, hop_samples=100)])
def test_half_precision_ring_rows(torch_cuda, kw):
    # the F16F16 ring format of the default widget: the half rows are the float rows rounded to nearest even (the 4096-point
    # and the mixed-radix kernels store them themselves, the others through a conversion pass)
    torch = torch_cuda
    kw = dict(dict(window_samples=W, hop_samples=H), **kw)
    eng = engine(**kw)
    n = eng.W + 40 * eng.H + 3
    pcm = to_dev(torch, oracle.white_noise(n * eng.channels, seed=3))
    f32 = eng.stft_batch(pcm)
    f16 = eng.stft_batch_f16(pcm)
    assert f16.dtype == torch.float16 and f16.shape == f32.shape
    assert torch.equal(f16, f32.to(torch.float16))
    part = eng.stft_batch_f16(pcm, first_frame=7, max_frames=9)
    assert torch.equal(part, f16[7:16])
    ref = oracle.stream_process(pcm.cpu().numpy(), eng.channels, eng.W, eng.H, threads=8)
    rel = np.abs(f16.cpu().numpy().astype(np.float64) - ref) / np.maximum(np.abs(ref), 0.05 * np.abs(ref).max())
    assert rel.max() < 1e-3  # half has an 11-bit significand


@pytest.mark.parametrize("period,Wexp", [(2048 / 48000.0 + 1e-7, 2048), (0.05, 2400)])
def test_cpp_host_mirror_program(torch_cuda, mags_err, tmp_path, period, Wexp):
    # include/sgx.hpp (C++ mirror of fourier::{AudioTransform, FastFourierTransform, AudioStreamTransform}) driven
    # by a compiled C++ program: ring -> hop loop -> frames, compared with the oracle
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run(["make", "-C", os.path.join(here, "cpp"), "-s"], check=True)
    out = str(tmp_path / "frames.bin")
    stride, n = 2.0 / 1024, Wexp + 6 * 93 + 40
    r = subprocess.run([os.path.join(here, "cpp", "host_mirror_test"), out, "48000", repr(period), repr(stride), str(n)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    frames, M_, Hs, left = np.frombuffer(raw[:32].tobytes(), dtype=np.uint64)
    assert (frames, M_, Hs) == (7, Wexp - 1, 93) and left == n - 8 * 93   # incl. the skip of the terminating read
    got = np.frombuffer(raw[32:].tobytes(), dtype=np.float32).reshape(int(frames), int(M_), 2)
    lr = oracle.white_noise(2 * n).reshape(-1, 2)
    ref = oracle.stream_process(lr, 2, Wexp, 93)
    assert mags_err(got, ref[:, 0]) <= (2.0 if Wexp == 2048 else 3.0)


def _turbo(t):
    # d3-scale-chromatic interpolateTurbo (the polynomial colorous::TURBO ports), clamped and rounded
    t = 0.0 if t != t else max(0.0, min(1.0, t))
    r = 34.61 + t * (1172.33 - t * (10793.56 - t * (33300.12 - t * (38394.49 - t * 14825.05))))
    g = 23.31 + t * (557.33 + t * (1225.33 - t * (3574.96 - t * (1073.77 + t * 707.56))))
    b = 27.2 + t * (3211.1 - t * (15327.97 - t * (27814.0 - t * (22569.18 - t * 6838.66))))
    return tuple(int(max(0, min(255, round(v)))) for v in (r, g, b))


def _diverging(t):
    # a three-stop diverging ramp (blue - white - red), linear in RGB, rounded: non-monotone per channel
    t = 0.0 if t != t else max(0.0, min(1.0, t))
    lo, mid, hi = (33, 102, 172), (247, 247, 247), (178, 24, 43)
    a, b, u = (lo, mid, t * 2) if t < 0.5 else (mid, hi, t * 2 - 1)
    return tuple(int(round(a[i] + (b[i] - a[i]) * u)) for i in range(3))


def test_continuous_gradients_through_a_callback(torch_cuda):
    # ColorScheme::new_mono / new_stereo with ANY colorous gradient: the colour function arrives as a
    # callback; its byte switch points become thresholds; bytes equal the oracle calling the same function
    torch = torch_cuda
    pcm = oracle.white_noise(2 * (W + 15 * H), seed=77).reshape(-1, 2) * np.array([1.0, 0.4], np.float32)
    mags = oracle.stream_process(pcm, 2, W, H)[:, 0]
    mags = (mags * np.logspace(-4, 1.5, 16, dtype=np.float32)[:, None, None]).astype(np.float32)
    mags[5] = 0.0
    dev = to_dev(torch, mags)
    eng = engine(window_samples=W, hop_samples=H, channels=2)
    try:
        for fn, stereo in ((_turbo, False), (_diverging, True), (_turbo, True)):
            eng.set_gradient_fn(fn, stereo=stereo)
            oracle.set_gradient_fn(fn)
            got = eng.render_mags(dev).cpu().numpy()
            ref = oracle.render_columns(mags, SR, None, stereo=stereo)
            assert np.array_equal(got, ref), (fn.__name__, stereo)
            assert len(np.unique(ref[..., :3].reshape(-1, 3), axis=0)) > 150
            assert np.array_equal(eng.lookup_table(32), oracle.lookup_table(None, 32, stereo=stereo))
        # end to end from PCM as well (two-kernel route for callback gradients)
        eng.set_gradient_fn(_turbo)
        oracle.set_gradient_fn(_turbo)
        x = to_dev(torch, pcm * np.float32(0.05))
        rg = eng.render_batch(x).cpu().numpy()[:, 0]
        own = oracle.render_columns(eng.stft_batch(x).cpu().numpy()[:, 0], SR, None)
        assert np.array_equal(rg, own)
        # the ColorScheme mirror routes callables the same way (Turbo = the d3 polynomial)
        from spectrogram_rs_amd import ColorScheme, default_color_schemes
        turbo = [c for c in default_color_schemes() if c.name == "Turbo"][0]
        turbo.apply(eng)
        oracle.set_gradient_fn(turbo.gradient_fn)
        assert np.array_equal(eng.render_mags(dev).cpu().numpy(), oracle.render_columns(mags, SR, None))
        assert turbo.foreground() == _turbo(1.0) and turbo.background() == _turbo(0.0)
        # a table set afterwards replaces the callback
        eng.set_builtin_gradient("viridis")
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz"))["viridis"]
        assert np.array_equal(eng.render_mags(dev).cpu().numpy(), oracle.render_columns(mags, SR, g))
    finally:
        oracle.set_gradient_fn(None)


@pytest.mark.parametrize("name,stereo", [("red_yellow_blue", True), ("red_blue", True), ("spectral", True), ("red_yellow_green", True),
                                         ("pink_green", True), ("purple_orange", True), ("cividis", False), ("cubehelix", False),
                                         ("turbo", False), ("cool", False), ("reds", False), ("blues", False), ("greens", False),
                                         ("greys", False), ("oranges", False)])
def test_builtin_continuous_schemes(torch_cuda, name, stereo):
    # every continuous entry of default_color_schemes (colorscheme.rs:129-149; the four 256-entry ramps have their own
    # tests): the library evaluates colorous' B-spline gradients (anchors from ColorBrewer, d3's interpolateRgbBasis), the
    # Turbo / Cividis polynomials and the cubehelix interpolations (Cube-helix, Cool) itself.  The pixel arithmetic is
    # checked against the oracle; the COLOUR function the oracle is handed is the checker's own restatement of the
    # published d3 formulas (oracle/gradients.py over tests/golden/brewer_anchors.npz -- nothing of it comes from the
    # product package).  It pins the engine's evaluation and thresholding of a gradient; about colorous itself
    # (unvendored) it says only what tests/test_host_logic.py::test_independent_pins_... lists.
    torch = torch_cuda
    from oracle.gradients import CONTINUOUS
    from spectrogram_rs_amd import ColorScheme
    from spectrogram_rs_amd.colorscheme import default_color_schemes
    from spectrogram_rs_amd.engine import builtin_gradient_eval
    pcm = oracle.white_noise(2 * (W + 15 * H), seed=78).reshape(-1, 2) * np.array([1.0, 0.3], np.float32)
    mags = oracle.stream_process(pcm, 2, W, H)[:, 0]
    mags = (mags * np.logspace(-4, 1.5, 16, dtype=np.float32)[:, None, None]).astype(np.float32)
    mags[3] = 0.0
    eng = engine(window_samples=W, hop_samples=H, channels=2)
    eng.set_builtin_scheme(name, stereo=stereo)
    try:
        oracle.set_gradient_fn(CONTINUOUS[name])
        got = eng.render_mags(to_dev(torch, mags)).cpu().numpy()
        assert np.array_equal(got, oracle.render_columns(mags, SR, None, stereo=stereo))
        assert np.array_equal(eng.lookup_table(32), oracle.lookup_table(None, 32, stereo=stereo))
        # PCM to pixels through the same entry point; the ColorScheme mirror picks the built-in by name
        scheme = [c for c in default_color_schemes() if c.builtin == name][0]
        assert scheme.is_stereo == stereo and scheme.foreground() == builtin_gradient_eval(name, 0.5 if stereo else 1.0)
        other = engine(window_samples=W, hop_samples=H, channels=2)
        scheme.apply(other)
        x = to_dev(torch, pcm * np.float32(0.05))
        assert torch.equal(other.render_batch(x), eng.render_batch(x))
    finally:
        oracle.set_gradient_fn(None)


@pytest.mark.parametrize("interp", [0, 1])
def test_magnitude_in_over_spectrum_analyzer_bands(torch_cuda, interp):
    # FrequencySample::magnitude_in (the pixel-stage boundary, src/fourier/mod.rs:17-21) over the 128 log-spaced
    # bands of SpectrumAnalyzer::push_frequencies (spectrum_analyzer.rs:20-61), bit-exact vs the oracle
    torch = torch_cuda
    start, end, nb = np.float32(32.0), np.float32(24000.0), 129
    ls, le = np.float32(np.log10(start)), np.float32(np.log10(end))
    step = np.float32((le - ls) / np.float32(nb))
    edges = np.array([np.float32(10.0) ** np.float32(ls + step * np.float32(i)) for i in range(nb + 1)], np.float32)
    ranges = np.stack([edges[:-1], edges[1:]], 1)[:128]
    ranges = np.concatenate([ranges, np.array([[0.0, 5.0], [23990.0, 24000.0], [100.0, 100.0], [5000.0, 4000.0]], np.float32)])
    eng = engine(window_samples=W, hop_samples=H, channels=2, interp=interp)
    mags = oracle.stream_process(oracle.white_noise(2 * (W + 5 * H), seed=12), 2, W, H)[:, 0]
    got = eng.magnitude_in(to_dev(torch, mags), ranges).cpu().numpy()
    ref = np.stack([[oracle.magnitude_in(m, SR, float(a), float(b), interp) for a, b in ranges] for m in mags])
    assert got.shape == ref.shape == (6, 132, 2) and np.array_equal(got, ref)
    # a different range set replaces the cached tables
    got2 = eng.magnitude_in(to_dev(torch, mags), ranges[:7]).cpu().numpy()
    assert np.array_equal(got2, ref[:, :7])


def test_lookup_table_and_widget_ring(torch_cuda, gradients):
    torch = torch_cuda
    from spectrogram_rs_amd import ColorScheme, RingBuffer, SimpleSpectrogram
    eng = engine(window_samples=W, hop_samples=H)
    cs = ColorScheme.new_mono("magma", "Magma")
    assert np.array_equal(cs.lookup_table(32, eng), oracle.lookup_table(gradients["magma"], 32))
    cs2 = ColorScheme.new_stereo(gradients["plasma"], (0, 0, 0), "Plasma (Stereo)")
    assert np.array_equal(cs2.lookup_table(32, eng), oracle.lookup_table(gradients["plasma"], 32, stereo=True))
    assert cs2.background() == (0, 0, 0) and cs.background() == tuple(gradients["magma"][0])
    # SimpleSpectrogram: columns land at offset, offset advances modulo width, low frequencies at the bottom
    rb = RingBuffer(1 << 20)
    w = SimpleSpectrogram(rb, sample_rate=48000, window_samples=W, width=64, height=R)
    w.set_palette(ColorScheme.new_mono("viridis", "Viridis"))
    H2 = w.engine.H
    t = np.arange(W + 9 * H2) / 48000.0
    tone = (0.25 * np.sin(2 * np.pi * 100.0 * t)).astype(np.float32)
    rb.push_mono(tone)
    assert w.snapshot() == 10 and w.offset == 10
    img = w.buffer.cpu().numpy()
    bg = gradients["viridis"][0]
    lit_rows = np.nonzero((img[:, 0, :3] != bg).any(axis=1))[0]
    assert len(lit_rows) and lit_rows.min() > R // 2 and (img[:, 10:, :] == 0).all()
    mags = oracle.stream_process(np.stack([tone, tone], 1), 2, W, H2)[:, 0]
    ref = oracle.render_columns(mags, 48000, gradients["viridis"])
    diff = (img[:, :10].transpose(1, 0, 2) != ref).any(axis=2).mean()
    assert diff < 5e-3
    assert w.scrolled().shape == (R, 64, 4)
