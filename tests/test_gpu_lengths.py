"""Every transform length the library accepts against the float64 truth (tests/length_sweep.py: the sets, derived from the plan rules
as the tests restate them; tests/test_length_sweep.py checks the sets on the CPU), all through the C ABI.

The transform length selects a plan built at run time -- stages, (RA, RB) pairs, twiddles, padding, split table, convolution length,
kernel 11's N1 x N2 and sub-transform radices -- and the other GPU files run a few dozen lengths by name.  Here each length gets a
context with 2 channels and one with 1 (rows = 16: small pixel tables), and first the route is asserted: stft_kernel and render_path bits 2
and 3 as the set records them.  Then, on three frames of white noise (hop W // 3 + 1, a ragged tail of H - 1 samples, seed W):

  magnitudes     every frame of stft_batch against edge_signals.truth_frame at the floor and bound of the kernel class
  sub-range      first_frame = 1, max_frames = 1 gives the bytes of row 1
  half rows      stft_batch_f16 is .half() of the rows
  complex rows   stft_batch_complex against test_gpu_complex.truth_complex at the same bound; moduli within HYPOT_ULPS of the magnitudes
  inverse        where istft_supported: istft_batch(stft_batch_complex(x)) is x within test_gpu_istft.ROUND_TRIP_TOL on the steady-state hop
                 [2H, 3H), whose H samples visit every position of a frame

Kernel 11 (SGX_FLAG_LARGE_TRANSFORM): 2 channels, two frames, magnitudes and the sub-range.  A case is a chunk of lengths; every length of
a chunk runs, whatever the ones before it did, and the case fails with the list of all that failed -- a length the library refuses
included.  A failing magnitude frame is reported with the ratio an independent float32 FFT reads on the same frame.
Measured ratios and wall times: profiles/r10_lengths.txt.  Run with -m gpu on an MI355X."""
import time

import numpy as np
import pytest

import edge_signals as es
import length_sweep as ls
import oracle
from conftest import chirpz_bound, mags_error
from test_gpu_complex import HYPOT_ULPS, complex_error, truth_complex
from test_gpu_istft import ROUND_TRIP_TOL
from test_gpu_large import LARGE_BOUND

pytestmark = pytest.mark.gpu

# Multiples of the floor a length is held to: those the kernel classes already have (conftest.KERNEL_BOUND through chirpz_bound for
# kernel 4, test_gpu_large.LARGE_BOUND for kernel 11, 1 x otherwise).  A class measured above 1 x by the protocol of
# profiles/r10_lengths.txt would be named here, beside test_gpu_edges.EDGE_BOUND; none was needed.
LENGTH_BOUND = {"default": 1.0}
CHUNKS = ls.chunks()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def bound(e):
    if e.kernel == 4:
        return chirpz_bound(e.W)
    return LARGE_BOUND["default"] if e.kernel == 11 else LENGTH_BOUND["default"]


def sweep_one(torch, e, channels, stats):
    """every check of one context; returns the list of failures (strings), empty when the length holds"""
    from spectrogram_rs_amd import SgxError, SpectrogramEngine
    W, H, large = e.W, e.H, e.kernel == 11
    tag = f"W {W} {'+'.join(e.flags) or 'default'} ch {channels}"
    try:
        eng = SpectrogramEngine(es.SR, device=0, **e.engine_kwargs(channels))
    except SgxError as err:
        return [f"{tag}: refused: {err}"]
    try:
        info = eng.info
        on, off = e.bits(channels)
        if info.stft_kernel != e.kernel or info.render_path & on != on or info.render_path & off:
            return [f"{tag}: route: stft_kernel {info.stft_kernel} render_path {info.render_path}, expected kernel {e.kernel}, bits "
                    f"set {on} clear {off}"]
        fails = []
        frames = 2 if large else 3
        pcm = ls.stream(e, channels, frames)
        dev = torch.from_numpy(pcm.reshape(-1)).cuda()
        rows_dev = eng.stft_batch(dev)
        rows = rows_dev.cpu().numpy()
        if rows.shape != (frames, 1, W - 1, 2):
            return [f"{tag}: {rows.shape} rows for {frames} frames"]
        paired = "paired_frames" in e.flags and channels == 1
        lrs = [es.frame_lr(pcm[t * H:t * H + W], 0) for t in range(frames)]
        # (kernel 11's windows are long and run once: their Hann tables stay out of edge_signals.hann's cache)
        win = oracle.hann_window(W) if large else es.hann(W)
        truths = [es.truth_frame(lr, W, win) for lr in lrs]
        peaks = [float(np.abs(t).max()) for t in truths]

        def partner(t):    # paired mono frames (2q, 2q + 1) share one transform: the allowance follows the larger peak
            return peaks[t ^ 1] if paired and (t ^ 1) < frames else 0.0

        for t in range(frames):
            r = es.pair_error(rows[t, 0], truths[t], e.floor, partner(t)) if paired else mags_error(rows[t, 0], truths[t], e.floor)
            stats["mags"] = max(stats["mags"], (r, W, channels, e.flags))
            if not r <= bound(e):
                ind = ls.independent_float32_ratio(lrs[t], W, e.floor)
                fails.append(f"{tag}: frame {t} magnitudes {r:.4f} x (bound {bound(e)}); an independent float32 FFT reads {ind:.4f} x")
        part = eng.stft_batch(dev, first_frame=1, max_frames=1).cpu().numpy()
        if not np.array_equal(part.view(np.uint32), rows[1:2].view(np.uint32)):
            fails.append(f"{tag}: the sub-range (1, 1) is not the bytes of row 1")
        if large:
            return fails
        if not torch.equal(eng.stft_batch_f16(dev), rows_dev.half()):
            fails.append(f"{tag}: half rows are not .half() of the rows")
        cx_dev = eng.stft_batch_complex(dev)
        cx = cx_dev.cpu().numpy()
        for t in range(frames):
            ref = truth_complex(lrs[t], W)
            r = complex_error(cx[t, 0], ref, e.floor, max(float(np.abs(ref).max()), partner(t)))
            stats["complex"] = max(stats["complex"], (r, W, channels, e.flags))
            if not r <= bound(e):
                fails.append(f"{tag}: frame {t} complex rows {r:.4f} x (bound {bound(e)})")
        m = rows.astype(np.float64)
        ulp = np.spacing(np.maximum(m, 2.0 ** -40).astype(np.float32)).astype(np.float64)
        r = float((np.abs(np.abs(cx.astype(np.complex128)) - m) / ulp).max())
        stats["hypot"] = max(stats["hypot"], (r, W, channels, e.flags))
        if not r <= HYPOT_ULPS:
            fails.append(f"{tag}: moduli {r:.2f} ulps from the magnitudes (bound {HYPOT_ULPS})")
        if eng.istft_supported() != 1:
            fails.append(f"{tag}: istft_supported is {eng.istft_supported()}")
            return fails
        y = eng.istft_batch(cx_dev)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        if y.shape != ((frames - 1) * H + W, channels):
            return fails + [f"{tag}: istft_batch returned {y.shape}"]
        # the steady-state hop of the run, [2H, 3H): sample 2H + j lies at position j of frame 2, H + j of frame 1 and (while inside the
        # window) 2H + j of frame 0 -- the H samples visit every position of a frame, all under the interior envelope of this hop, where
        # test_gpu_istft holds its round trip to ROUND_TRIP_TOL of the local peak
        lo, hi = (frames - 1) * H, frames * H
        assert hi - lo == H and hi > W and H <= W // 2
        d = np.abs(y[lo:hi].astype(np.float64) - pcm[lo:hi])
        r = float((d / (ROUND_TRIP_TOL * np.maximum(ls.local_peak_at(pcm, W, lo, hi), 1e-30))).max())
        stats["round trip"] = max(stats["round trip"], (r, W, channels, e.flags))
        stats["held"] = stats.get("held", 0) + (hi - lo) * channels
        if not r <= 1.0:
            fails.append(f"{tag}: round trip {r:.3f} of its bound")
        return fails
    finally:
        eng.close()


@pytest.mark.parametrize("chunk", list(CHUNKS))
def test_lengths(torch_cuda, chunk):
    t0 = time.perf_counter()
    stats = {k: (0.0, 0, 0, ()) for k in ("mags", "complex", "hypot", "round trip")}
    fails, contexts = [], 0
    for e in CHUNKS[chunk]:
        for channels in e.channels:
            fails += sweep_one(torch_cuda, e, channels, stats)
            contexts += 1
    held = stats.pop("held", 0)
    worst = ", ".join(f"{k} {v[0]:.4f} (W {v[1]} ch {v[2]}{' ' + '+'.join(v[3]) if v[3] else ''})" for k, v in stats.items() if v[1])
    worst += f"; round trip held on {held} samples" if held else ""
    print(f"LENGTHS {chunk}: {len(CHUNKS[chunk])} lengths, {contexts} contexts, {time.perf_counter() - t0:.2f} s; worst {worst}")
    assert not fails, "\n".join([f"{len(fails)} failures in {chunk}:"] + fails)
