"""sgx_flux_batch / sgx_flux_mags: per band the rise and the fall of every bin against the same bin `lag` frames earlier
(include/sgx.h), through the C ABI.

The contract is that a record is a pure function of two rows and the bank: the stage call equals tests/flux_reference.py (one float32
subtract, two selects, the filterbank sums' order) bit for bit on crafted rows on both sides of the kernel's LDS decision; the batch call
equals the stage call over the same call's sgx_stft_batch rows, and the reference, bit for bit on every transform family -- for any
first_frame and split of the call, across the workspace's range seam, at any compute-unit limit, run claim and stream.  Every output
buffer is NaN before the call and sits between guard words.

Two bounds appear, both derived:
  - stage output against the float64 flux of the same float32 rows: (ceil(count / 64) + 9) 2^-24 sum |w| (x_t + x_{t - lag}) -- one
    rounding for the square, one for the subtract, the chain, six tree levels, one unit for second order;
  - batch output (power 1) against the flux of the float64 truth rows: sum |w| (allow_t + allow_{t - lag}) plus the bound above, allow the
    per-bin allowance of tests/conftest.py with the family's floor -- rectification is 1-Lipschitz, so a row error passes through it
    undiminished at most."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_signals as es
import fbank_reference as fr
import flux_reference as ref
import stream_cases
from conftest import REL_TOL
from spectrogram_rs_amd import SpectrogramEngine, _lib, mel_weights

pytestmark = pytest.mark.gpu

SR = 48000.0
LAGS = (1, 2, 5, 64)
GUARD = 64                            # floats before and after every output: 256 bytes, so the output stays 16-byte aligned
WORKSPACE_BYTES = 192 << 20           # include/sgx.h: the bounded workspace


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def vp(t):
    return C.c_void_p(t.data_ptr())


def lds_optin():
    hip = C.CDLL("libamdhip64.so")
    optin = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(optin), 75, 0) == 0      # hipDeviceAttributeSharedMemPerBlockOptin
    return optin.value


class Guarded:
    """n floats of NaN between two runs of GUARD floats of NaN"""

    def __init__(self, eng, n):
        import torch

        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
        self.stale = bits(self.buf)
        self.out = self.buf[GUARD:GUARD + n]

    def guards_untouched(self):
        now = bits(self.buf)
        return np.array_equal(now[:GUARD], self.stale[:GUARD]) and np.array_equal(now[GUARD + self.n:], self.stale[GUARD + self.n:])

    def untouched(self):
        return np.array_equal(bits(self.buf), self.stale)


def stage(fb, rows, lag):
    """sgx_flux_mags over float32 rows [frames][pairs][M][2] on the device -> [frames][pairs][n_filters][4], guards checked"""
    import torch

    eng = fb.engine
    eng.use_current_stream()
    n = rows.numel() // (eng.pairs * eng.M * 2)
    g = Guarded(eng, n * eng.pairs * fb.n_filters * 4)
    eng._check(eng._lib.sgx_flux_mags(fb._h, vp(rows), n, C.c_uint32(lag), vp(g.out)))
    torch.cuda.current_stream().synchronize()
    assert g.guards_untouched(), "sgx_flux_mags wrote outside its output"
    return g.out.view(n, eng.pairs, fb.n_filters, 4)


def batch(fb, pcm, lag, first_frame=0, max_frames=None):
    """sgx_flux_batch -> [frames][pairs][n_filters][4], *n_out and the guards checked"""
    import torch

    eng = fb.engine
    eng.use_current_stream()
    n_samples = pcm.numel() // eng.channels
    n = max(eng.num_frames(n_samples) - first_frame, 0)
    if max_frames is not None:
        n = min(n, max_frames)
    g = Guarded(eng, n * eng.pairs * fb.n_filters * 4)
    got = C.c_size_t(7)
    eng._check(eng._lib.sgx_flux_batch(fb._h, vp(pcm), n_samples, first_frame, 2 ** 40 if max_frames is None else max_frames,
                                             C.c_uint32(lag), vp(g.out), C.byref(got)))
    torch.cuda.current_stream().synchronize()
    assert got.value == n
    assert g.guards_untouched(), "sgx_flux_batch wrote outside its output"
    return g.out.view(n, eng.pairs, fb.n_filters, 4)


def assert_records(got, want, what):
    """bit for bit; where the reference is NaN the device is NaN (the payload is unspecified)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in {int(np.isnan(got).sum())} words, the definition has {int(nan.sum())}"
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    if not np.array_equal(g, w):
        idx = tuple(int(i) for i in np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} words differ from the definition; first at (frame, pair, filter, "
                             f"component) {idx}: device {float(got[idx])!r}, definition {float(want[idx])!r}")


# ---- 1: the stage call on crafted rows -----------------------------------------------------------------------------------------------------
STAGE_CONTEXTS = {   # name: (engine keyword arguments, M).  Four channels: the pair stride is live.  M 10 240 | 10 241: the LDS decision
    "m3": (dict(window_samples=4, hop_samples=1, channels=4), 3),
    "m63": (dict(window_samples=64, hop_samples=16, channels=4), 63),
    "m64": (dict(window_samples=65, hop_samples=16, channels=4), 64),
    "m65": (dict(window_samples=66, hop_samples=16, channels=4), 65),
    "m2047": (dict(window_samples=2048, hop_samples=256, channels=4), 2047),
    "m10240": (dict(window_samples=10241, hop_samples=5000, channels=2, large_transforms=True), 10240),
    "m10241": (dict(window_samples=10242, hop_samples=5000, channels=2, large_transforms=True), 10241),
}


def crafted_rows(pairs, M, lag, seed):
    """lag + 6 frames of synthetic magnitudes with the definition's cases on them: a row of zeros as a predecessor (row 0, of frame lag)
    and as a frame between two others (lag + 2), a frame equal to its predecessor (lag + 1: all four +0), a NaN bin (frame lag + 4)"""
    frames = lag + 6
    rows = fr.synthetic_mags(frames * pairs, M, seed).reshape(frames, pairs, M, 2).copy()
    assert fr.zero_or_normal(rows)
    rows[0] = 0.0
    rows[lag + 1] = rows[1]
    rows[lag + 2] = 0.0
    rows[lag + 4, pairs - 1, M // 2, 0] = np.nan
    return rows


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("name", list(STAGE_CONTEXTS))
def test_stage_on_crafted_rows(name, lag):
    import torch

    kw, M = STAGE_CONTEXTS[name]
    eng = SpectrogramEngine(SR, device=0, **kw)
    try:
        assert eng.M == M and eng.pairs == kw["channels"] // 2
        if M >= 10240:
            cap = lds_optin()
            assert cap >= fr.STAGE_LDS_CAP, f"this device offers {cap} bytes of LDS: the lengths here no longer lie on both sides of the decision"
            assert ref.flux_stage_staged(M, cap) == (M == 10240)
        rows = crafted_rows(eng.pairs, M, lag, seed=1000 * lag + M)
        dev = torch.from_numpy(rows).to(eng.device)
        banks = {"edges": fr.edge_bank(M), "ones": ref.ones_bank(M), "empty": ref.empty_bank(M)}
        for kind, bank in banks.items():
            for power in (1, 2):
                fb = eng.filterbank(*bank, power=power)
                want = ref.flux(rows, bank, power, lag)
                for n in sorted({1, lag, lag + 1, lag + 6}):
                    got = stage(fb, dev[:n].contiguous(), lag).cpu().numpy()
                    assert_records(got, want[:n], f"{name}/{kind}/power {power}/lag {lag}/{n} frames")
                    assert not got[:lag].view(np.uint32).any(), "a frame without a predecessor is not +0"
                if kind == "empty":
                    assert not want.view(np.uint32).any()
                else:
                    w = want.view(np.uint32)
                    assert not w[lag + 1].any(), "equal rows: not +0 in all four (by bit pattern)"
                    covered = (bank[0] <= M // 2) & (M // 2 < bank[0].astype(np.int64) + bank[1])
                    assert np.isnan(want[lag + 4, eng.pairs - 1, covered][:, [0, 2]]).all() and not np.isnan(want[lag + 4, eng.pairs - 1, ~covered]).any()
                    assert not np.isnan(want[lag + 4, eng.pairs - 1][:, [1, 3]]).any(), "the NaN of the left side reached the right"
                    assert (want[lag + 2][..., :2] == 0).all() and (want[lag][..., 2:] == 0).all()      # into silence: no rise; out of it: no fall
                fb.close()
    finally:
        eng.close()


# ---- 2: the batch call on one context per transform family -------------------------------------------------------------------------------
FAMILY_ROUTES = {   # label: (row of tests/edge_signals.py: ROUTES, family of tests/stream_cases.py, frames)
    "wg4096_real_h256": ("k1r_h256", "wg4096", 40),
    "wg4096_lr": ("k1_lr_h256", "wg4096", 40),
    "wg4096_ch4": ("k1_ch4", "wg4096", 40),
    "w4800": ("k48_lr", "w4800", 40),
    "mixed": ("mixed_w1024_lr", "mixed", 40),
    "chirpz": ("chirpz_w1102_lr", "chirpz", 40),
    "bluestein": ("bluestein_w1102", "bluestein", 40),
    "generic": ("generic_w256_lr", "generic", 40),
    "w16384": ("k16_lr_h512", "w16384", 24),
    "large": ("large_w19200_lr", "large", 24),
}


def tones_in_noise(eng, frames, seed):
    """the engine's white noise at 0.1 plus two tones per channel that start and stop: onsets and offsets for the flux to see"""
    import torch

    n = eng.W + (frames - 1) * eng.H
    t = torch.arange(n, dtype=torch.float64, device=eng.device)
    pcm = 0.1 * eng.white_noise(n, seed=seed).view(n, eng.channels)
    for c in range(eng.channels):
        for amp, frac, lo, hi in ((0.5, 0.123 + 0.01 * c, 0.2, 0.7), (0.3, 0.371 - 0.01 * c, 0.45, 1.0)):
            gate = ((t >= lo * n) & (t < hi * n)).double()
            pcm[:, c] += (amp * gate * torch.cos(np.pi * frac * t)).float()
    return pcm.reshape(-1).contiguous()


@functools.lru_cache(maxsize=None)
def family_context(label):
    """one engine per family with its stream, its own sgx_stft_batch rows on the device and on the host: made once, never written to"""
    import torch

    name, fam, frames = FAMILY_ROUTES[label]
    r = es.ROUTE[name]
    assert stream_cases.family(r) == fam
    eng = SpectrogramEngine(SR, device=0, **r.engine_kwargs())
    assert eng.info.stft_kernel == r.kernel, f"{label}: kernel {eng.info.stft_kernel}, the route table says {r.kernel}"
    assert eng.info.render_path & r.bits_set == r.bits_set and not eng.info.render_path & r.bits_clear
    pcm = tones_in_noise(eng, frames, seed=0xF1A7 + len(label))
    rows = eng.stft_batch(pcm)
    torch.cuda.synchronize()
    host = rows.cpu().numpy()
    host.setflags(write=False)
    return eng, pcm, rows, host


@functools.lru_cache(maxsize=None)
def family_bank(label, kind):
    """(bank arrays, power, the FilterBank on the family's engine)"""
    eng = family_context(label)[0]
    bank, power = (mel_weights(SR, eng.W, 128, 0.0, SR / 2), 2) if kind == "mel128" else (fr.edge_bank(eng.M), 1)
    return bank, power, eng.filterbank(*bank, power=power)


@pytest.mark.parametrize("kind", ["mel128", "edges"])
@pytest.mark.parametrize("label", sorted(FAMILY_ROUTES))
def test_batch_on_every_family(label, kind):
    eng, pcm, rows, host = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    bank, power, fb = family_bank(label, kind)
    assert fb.flux_max_lag == 64
    for lag in (1, 3):
        got = batch(fb, pcm, lag)
        assert got.shape == (frames, eng.pairs, fb.n_filters, 4)
        staged = stage(fb, rows, lag)
        assert np.array_equal(bits(got), bits(staged)), f"{label}/{kind}/lag {lag}: the batch call differs from the stage call over its own rows"
        assert_records(got.cpu().numpy(), ref.flux(host, bank, power, lag), f"{label}/{kind}/lag {lag}")
        g = got.cpu().numpy()
        assert not g[:lag].view(np.uint32).any() and g[lag:, :, bank[1] > 0].any(axis=(0, 1, 2)).all()      # rises and falls both occur
        if eng.channels == 1:
            assert np.array_equal(np_bits(g[..., 0]), np_bits(g[..., 1])) and np.array_equal(np_bits(g[..., 2]), np_bits(g[..., 3])), \
                f"{label}: a mono stream does not hold rise_l = rise_r"


# ---- 3: first_frame and splits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [1, 5])
@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "w4800", "generic", "w16384"])
def test_first_frame_and_splits(label, lag):
    eng, pcm, rows, host = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    bank, power, fb = family_bank(label, "mel128")
    full = batch(fb, pcm, lag)
    whole = bits(full).reshape(frames, -1)
    assert not whole[:lag].any() and whole[lag:].any(axis=1).all(), "zero records exactly for the frames t < lag"
    for first in sorted({0, 1, lag - 1, lag, lag + 1, 17}):
        part = batch(fb, pcm, lag, first_frame=first)
        assert np.array_equal(bits(part), whole[first:].reshape(-1)), f"{label}/lag {lag}: first_frame {first}"
        short = batch(fb, pcm, lag, first_frame=first, max_frames=3)
        assert np.array_equal(bits(short), whole[first:first + 3].reshape(-1)), f"{label}/lag {lag}: frames {first} .. {first + 2}"
    # splits inside the first `lag` frames, at `lag` itself and beyond
    for cuts in ([1], [lag], [lag + 1], [2, 4, 7], [1, 2, 3, 4, 5, 6, 21]):
        edges = [0] + [c for c in cuts if c < frames] + [frames]
        parts = [batch(fb, pcm, lag, first_frame=a, max_frames=b - a) for a, b in zip(edges, edges[1:]) if b > a]
        assert np.array_equal(np.concatenate([bits(p) for p in parts]), whole.reshape(-1)), f"{label}/lag {lag}: split at {cuts}"


# ---- 4: the range seam ----------------------------------------------------------------------------------------------------------------------
def test_range_seam_at_w8192_ch8():
    """W 8192 with 8 channels: a frame's rows are 262 112 bytes, 768 frames' rows fit the workspace; 800 frames at lag 64 take two ranges,
    the second with a head of 64 recomputed rows"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=8192, hop_samples=64, channels=8)
    frames, lag = 800, 64
    cap = WORKSPACE_BYTES // (eng.pairs * eng.M * 8)
    assert cap == 768 and frames > cap
    bank = mel_weights(SR, eng.W, 128, 0.0, SR / 2)
    fb = eng.filterbank(*bank, power=2)
    assert fb.flux_max_lag == 64
    pcm = tones_in_noise(eng, frames, seed=99)
    rows = eng.stft_batch(pcm)
    got = batch(fb, pcm, lag)
    staged = stage(fb, rows, lag)
    assert torch.equal(got.view(torch.int32), staged.view(torch.int32)), "the batch call across the range seam differs from the stage call"
    assert not got[:lag].any().item() and got[lag:].any(dim=-1).any(dim=-1).all().item()
    seam = cap                                                                    # the first frame of the second range
    ts = [seam - 1, seam, seam + 1, seam + 17, frames - 1]
    assert all(lag <= t < frames for t in ts)
    frame = lambda t, src: src[t].cpu().numpy()                                  # (one frame at a time: plain copies, no gather on the device)
    want = ref.flux_of(np.stack([frame(t, rows) for t in ts]), np.stack([frame(t - lag, rows) for t in ts]), bank, 2)
    assert_records(np.stack([frame(t, got) for t in ts]), want, "frames either side of the seam")
    parts = [batch(fb, pcm, lag, max_frames=seam + 1), batch(fb, pcm, lag, first_frame=seam + 1)]
    assert torch.equal(torch.cat(parts).view(torch.int32), got.view(torch.int32))
    fb.close()
    eng.close()


# ---- 5: independence of compute-unit limit, run claim, stream and channel count -----------------------------------------------------------
@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "wg4096_ch4", "w4800", "w16384"])
def test_cu_limits(label):
    import torch

    eng, pcm, _, _ = family_context(label)
    _, _, fb = family_bank(label, "mel128")
    lag = 3
    try:
        expect = bits(batch(fb, pcm, lag))
        for limit in (1, 3, 255):
            eng.set_cu_limit(limit)
            assert np.array_equal(bits(batch(fb, pcm, lag)), expect), f"{label}: {limit} compute units"
            part = batch(fb, pcm, lag, first_frame=7, max_frames=9)
            assert np.array_equal(bits(part), expect.reshape(FAMILY_ROUTES[label][2], -1)[7:16].reshape(-1)), f"{label}: frames 7 .. 15 at {limit}"
    finally:
        eng.set_cu_limit(0)
    torch.cuda.synchronize()


def test_run_claims_on_the_mono_w2048_context():
    eng, pcm, _, _ = family_context("wg4096_real_h256")
    _, _, fb = family_bank("wg4096_real_h256", "mel128")
    lag = 2
    try:
        eng.set_run_claim(16, 0)
        static = bits(batch(fb, pcm, lag))
        eng.set_run_claim(4, 8)
        claimed = bits(batch(fb, pcm, lag))
        eng.set_run_claim(0, 0)
        eng.set_run_weights((100, 80, 50, 26))
        weighted = bits(batch(fb, pcm, lag))
    finally:
        eng.set_run_claim(0, 0)
        eng.set_run_weights(None)
    assert np.array_equal(static, claimed) and np.array_equal(static, weighted)
    assert np.array_equal(static, bits(batch(fb, pcm, lag)))


@pytest.mark.parametrize("label", sorted(FAMILY_ROUTES))
def test_stream_ordered_and_asynchronous(label):
    """Both calls on every transform family, queued behind a long kernel on a non-default stream: they return before that kernel ends; the
    input is written on the same stream behind the sleep and is NaN until then, the rows the stage call reads are made there too, so a
    kernel put on any other stream would difference NaNs.  (tests/test_gpu_stream_routes.py sweeps the other entry points this way; the
    flux calls are held to it here.)"""
    import torch

    r = es.ROUTE[FAMILY_ROUTES[label][0]]
    eng = SpectrogramEngine(SR, device=0, **r.engine_kwargs())
    frames, lag = 23, 2
    n = eng.W + (frames - 1) * eng.H
    fb = eng.filterbank(*mel_weights(SR, eng.W, 128, 0.0, SR / 2), power=2)
    want = bits(batch(fb, eng.white_noise(n, seed=21), lag))                          # the NULL stream; the workspace is grown here
    batch(fb, eng.white_noise(n, seed=22), lag)                                       # the workspace holds another stream's rows
    torch.cuda.synchronize()
    pcm = torch.full((n * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
    rows = torch.full((frames, eng.pairs, eng.M, 2), float("nan"), dtype=torch.float32, device=eng.device)
    g, gs = Guarded(eng, frames * eng.pairs * fb.n_filters * 4), Guarded(eng, frames * eng.pairs * fb.n_filters * 4)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    eng.set_stream(s.cuda_stream)
    lib, got = eng._lib, C.c_size_t(0)
    with torch.cuda.stream(s):
        torch.cuda._sleep(400_000_000)
    eng._check(lib.sgx_synth_white_noise(eng._ctx, vp(pcm), 0, n, eng.channels, 21))
    eng._check(lib.sgx_flux_batch(fb._h, vp(pcm), n, 0, frames, C.c_uint32(lag), vp(g.out), C.byref(got)))
    eng._check(lib.sgx_stft_batch(eng._ctx, vp(pcm), n, 0, frames, vp(rows), None))
    eng._check(lib.sgx_flux_mags(fb._h, vp(rows), frames, C.c_uint32(lag), vp(gs.out)))
    done = torch.cuda.Event()
    done.record(s)
    assert not done.query(), f"{label}: a flux call waited for the stream"
    eng.sync()
    assert got.value == frames and g.guards_untouched() and gs.guards_untouched()
    assert np.array_equal(bits(g.out), want), f"{label}: sgx_flux_batch on a held stream"
    assert np.array_equal(bits(gs.out), want), f"{label}: sgx_flux_mags on a held stream"
    eng.set_stream(0)
    fb.close()
    eng.close()


def test_six_channels():
    """three pairs: each pair is differenced against itself"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=256, channels=6)
    assert eng.pairs == 3
    frames, lag = 12, 2
    pcm = tones_in_noise(eng, frames, seed=6)
    bank = mel_weights(SR, eng.W, 128, 0.0, SR / 2)
    fb = eng.filterbank(*bank, power=2)
    got = batch(fb, pcm, lag)
    rows = eng.stft_batch(pcm)
    assert np.array_equal(bits(got), bits(stage(fb, rows, lag)))
    host = rows.cpu().numpy()
    assert_records(got.cpu().numpy(), ref.flux(host, bank, 2, lag), "six channels")
    assert not np.array_equal(bits(got[:, 0]), bits(got[:, 1])) and not np.array_equal(bits(got[:, 1]), bits(got[:, 2]))
    torch.cuda.synchronize()
    fb.close(), eng.close()


# ---- 6: meaning --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("lag", [1, 3])
def test_a_click_in_silence(channels, lag):
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=256, channels=channels)
    W, H, frames = eng.W, eng.H, 30
    n = W + (frames - 1) * H
    n0 = 3 * W + 37                                                               # no two frames see it under the same weight
    x = np.zeros((n, channels), np.float32)
    x[n0] = 0.5
    bank = mel_weights(SR, W, 128, 0.0, SR / 2)
    live = bank[1] > 0
    fb = eng.filterbank(*bank, power=2)
    got = batch(fb, torch.from_numpy(x.reshape(-1)).to(eng.device), lag).cpu().numpy()
    win = eng.window().astype(np.float64)

    def weight(t):
        o = n0 - t * H
        return float(win[o]) if t >= 0 and 0 <= o < W else 0.0

    seen = {"silent": 0, "entering": 0, "leaving": 0}
    for t in range(frames):
        w_t, w_p = weight(t), weight(t - lag)
        margin = 2.0 * REL_TOL * (w_t + w_p)                                     # the rows' own relative allowance, on both rows, squared
        if t < lag or (w_t == 0.0 and w_p == 0.0):
            assert not got[t].view(np.uint32).any(), f"frame {t}: no click in either window, yet not +0 in all four"
            seen["silent"] += 1
        elif w_t - w_p > margin:
            for s in range(2):
                assert (got[t, 0, live, s] > 0).all() and not got[t, 0, :, 2 + s].view(np.uint32).any(), \
                    f"frame {t}, side {s}: the click is entering, yet rise > 0 = fall does not hold"
            seen["entering"] += 1
        elif w_p - w_t > margin:
            for s in range(2):
                assert (got[t, 0, live, 2 + s] > 0).all() and not got[t, 0, :, s].view(np.uint32).any(), \
                    f"frame {t}, side {s}: the click is leaving, yet fall > 0 = rise does not hold"
            seen["leaving"] += 1
        if channels == 1:
            assert np.array_equal(np_bits(got[t, :, :, [0, 2]]), np_bits(got[t, :, :, [1, 3]])), "a mono stream holds (v, v)"
    assert seen["silent"] >= 10 and seen["entering"] >= 3 and seen["leaving"] >= 3, seen
    fb.close()
    eng.close()


@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "w4800", "generic"])
def test_against_the_float64_truth(label):
    eng, pcm, rows, host = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    floor = es.ROUTE[FAMILY_ROUTES[label][0]].floor
    bank = mel_weights(SR, eng.W, 128, 0.0, SR / 2)
    fb = eng.filterbank(*bank, power=1)
    x = pcm.cpu().numpy().reshape(-1, eng.channels)
    win = es.hann(eng.W)
    truth = np.stack([np.stack([es.truth_frame(es.frame_lr(x[t * eng.H:t * eng.H + eng.W], p), eng.W, win) for p in range(eng.pairs)])
                      for t in range(frames)])                                    # [frames][pairs][M][2] float64
    peak = np.abs(truth).max(axis=(-1, -2), keepdims=True)
    allow = REL_TOL * np.maximum(np.abs(truth), floor * peak)
    first, count, weights = bank
    off = fr._offsets(count)
    for lag in (1, 3):
        got = batch(fb, pcm, lag).cpu().numpy().astype(np.float64)
        want = ref.flux_float64(truth, bank, 1, lag)
        carried = np.zeros(got.shape[:3] + (2,))
        s = np.zeros_like(allow)
        s[lag:] = allow[lag:] + allow[:-lag]
        for f in range(len(first)):
            carried[:, :, f, :] = np.einsum("i,tpiq->tpq", np.abs(weights[off[f]:off[f + 1]].astype(np.float64)), s[:, :, first[f]:first[f] + count[f], :])
        bound = carried + ref.arithmetic_bound(host, bank, 1, lag)
        bound4 = np.concatenate([bound, bound], -1)
        err = np.abs(got - want)
        nz = bound4 > 0
        worst = float((err[nz] / bound4[nz]).max())
        print(f"{label}/lag {lag}: worst |got - flux of the truth| / bound = {worst:.3f}")
        assert (err <= bound4).all(), f"{label}/lag {lag}: {worst:.3f} x the bound"
    fb.close()


@pytest.mark.parametrize("name", ["m3", "m2047"])
def test_arithmetic_bound_on_the_stage(name):
    import torch

    kw, M = STAGE_CONTEXTS[name]
    eng = SpectrogramEngine(SR, device=0, **kw)
    bank = fr.edge_bank(M)
    for lag in (1, 3):
        rows = fr.synthetic_mags((lag + 4) * eng.pairs, M, 77 + lag).reshape(lag + 4, eng.pairs, M, 2)
        dev = torch.from_numpy(rows).to(eng.device)
        for power in (1, 2):
            fb = eng.filterbank(*bank, power=power)
            got = stage(fb, dev, lag).cpu().numpy().astype(np.float64)
            bound = ref.arithmetic_bound(rows, bank, power, lag)
            bound4 = np.concatenate([bound, bound], -1)
            err = np.abs(got - ref.flux_float64(rows, bank, power, lag))
            nz = bound4 > 0
            worst = float((err[nz] / bound4[nz]).max())
            print(f"{name}/lag {lag}/power {power}: worst |got - float64| / bound = {worst:.3f}")
            assert (err <= bound4).all(), f"{name}/lag {lag}/power {power}: {worst:.3f} x the arithmetic bound"
            fb.close()
    eng.close()


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch

    eng, pcm, rows, _ = family_context("wg4096_lr")
    frames = FAMILY_ROUTES["wg4096_lr"][2]
    _, _, fb = family_bank("wg4096_lr", "mel128")
    n = pcm.numel() // eng.channels
    lib, bad = eng._lib, _lib.SGX_ERR_INVALID_ARG
    g = Guarded(eng, frames * eng.pairs * fb.n_filters * 4)
    out, off = vp(g.out), C.c_void_p(g.out.data_ptr() + 4)
    u = C.c_uint32
    got = C.c_size_t(7)

    def batch_call(bank=fb._h, d_pcm=vp(pcm), lag=2, d_out=out):
        return lib.sgx_flux_batch(bank, d_pcm, n, 0, 1000, u(lag), d_out, C.byref(got))

    def stage_call(bank=fb._h, d_mags=vp(rows), lag=2, d_out=out):
        return lib.sgx_flux_mags(bank, d_mags, frames, u(lag), d_out)

    for call, who in ((batch_call, b"sgx_flux_batch"), (stage_call, b"sgx_flux_mags")):
        for kw in (dict(lag=0), dict(lag=65), dict(lag=2 ** 32 - 1), dict(d_out=off), dict(d_out=None),
                   {"d_pcm" if call is batch_call else "d_mags": None}):
            got.value = 7
            assert call(**kw) == bad, (who, kw)
            assert who in lib.sgx_last_error(eng._ctx), (who, kw, lib.sgx_last_error(eng._ctx))
            assert call is stage_call or got.value == 0
        got.value = 7
        assert call(bank=None) == bad and (call is stage_call or got.value == 0)
    assert b"aligned" in (batch_call(d_out=off), lib.sgx_last_error(eng._ctx))[1]
    assert b"aligned" in (stage_call(d_out=off), lib.sgx_last_error(eng._ctx))[1]
    assert lib.sgx_flux_max_lag(None) == 0 and lib.sgx_flux_max_lag(fb._h) == 64
    # not errors: too few samples, no frame in range, no frames, a null n_out
    got.value = 7
    assert lib.sgx_flux_batch(fb._h, vp(pcm), eng.W - 1, 0, 10, u(2), out, C.byref(got)) == 0 and got.value == 0
    got.value = 7
    assert lib.sgx_flux_batch(fb._h, vp(pcm), n, frames, 10, u(2), out, C.byref(got)) == 0 and got.value == 0
    assert lib.sgx_flux_mags(fb._h, vp(rows), 0, u(2), out) == 0
    torch.cuda.synchronize()
    assert g.untouched(), "a refused or empty call wrote to its buffer"
    assert lib.sgx_flux_batch(fb._h, vp(pcm), n, 0, 1000, u(2), out, None) == 0
    torch.cuda.synchronize()
    assert g.guards_untouched() and np.array_equal(bits(g.out), bits(batch(fb, pcm, 2)))


def test_a_bank_that_outlives_its_context():
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=256, channels=2)
    lib = eng._lib
    first, count, weights = mel_weights(SR, eng.W, 128, 0.0, SR / 2)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    eng._check(lib.sgx_fbank_create(eng._ctx, len(first), p(first), p(count), p(weights), 2, C.byref(h)))
    pcm = eng.white_noise(eng.W + 2 * eng.H, seed=3)
    n = pcm.numel() // eng.channels
    g = Guarded(eng, 3 * len(first) * 4)
    got = C.c_size_t(0)
    assert lib.sgx_flux_max_lag(h) == 64
    assert lib.sgx_flux_batch(h, vp(pcm), n, 0, 3, C.c_uint32(1), vp(g.out), C.byref(got)) == 0 and got.value == 3
    torch.cuda.synchronize()
    rows = eng.stft_batch(pcm)
    torch.cuda.synchronize()
    eng.close()                                                                   # sgx_destroy: the bank is detached
    g = Guarded(eng, 3 * len(first) * 4)
    bad = _lib.SGX_ERR_INVALID_ARG
    got.value = 7
    assert lib.sgx_flux_batch(h, vp(pcm), n, 0, 3, C.c_uint32(1), vp(g.out), C.byref(got)) == bad and got.value == 0
    assert lib.sgx_flux_mags(h, vp(rows), 3, C.c_uint32(1), vp(g.out)) == bad
    assert lib.sgx_flux_max_lag(h) == 0
    torch.cuda.synchronize()
    assert g.untouched()
    lib.sgx_fbank_destroy(h)


def test_the_cap_at_w_2_pow_20():
    """a frame's rows are 8 MiB less 8 bytes: 24 of them fit the workspace, so a frame and its predecessor lie 23 apart at most.  No
    transform runs here: the refusal comes before anything is enqueued"""
    import torch

    r = es.ROUTE["large_w1m_lr"]
    eng = SpectrogramEngine(SR, device=0, **r.engine_kwargs())
    assert eng.W == 1 << 20 and eng.channels == 2
    bank = ref.ones_bank(eng.M)
    fb = eng.filterbank(*bank, power=2)
    assert fb.flux_max_lag == 23 == ref.max_lag(eng.pairs * eng.M * 8)
    n = eng.W                                                                     # one frame
    pcm = torch.zeros(n * 2, dtype=torch.float32, device=eng.device)
    g = Guarded(eng, 4)
    got = C.c_size_t(7)
    rc = eng._lib.sgx_flux_batch(fb._h, vp(pcm), n, 0, 1, C.c_uint32(24), vp(g.out), C.byref(got))
    assert rc == _lib.SGX_ERR_UNSUPPORTED and got.value == 0
    msg = eng._lib.sgx_last_error(eng._ctx)
    assert b"sgx_flux_batch" in msg and b"23" in msg and b"sgx_flux_mags" in msg, msg
    torch.cuda.synchronize()
    assert g.untouched()
    fb.close()
    eng.close()


# ---- 8: python ------------------------------------------------------------------------------------------------------------------------------
def test_python_methods():
    eng, pcm, rows, host = family_context("wg4096_ch4")
    bank, power, fb = family_bank("wg4096_ch4", "mel128")
    assert fb.flux_max_lag == 64
    got = fb.flux_batch(pcm, lag=3, first_frame=2, max_frames=5)
    assert got.shape == (5, eng.pairs, fb.n_filters, 4)
    want = ref.flux_of(host[2:7], np.concatenate([np.zeros_like(host[:1]), host[:4]]), bank, power)
    want[0] = 0.0                                                                 # frame 2 < lag: no predecessor
    assert_records(got.cpu().numpy(), want, "flux_batch")
    whole = fb.flux_apply(rows, lag=3)
    assert whole.shape == (FAMILY_ROUTES["wg4096_ch4"][2], eng.pairs, fb.n_filters, 4)
    assert np.array_equal(bits(whole[2:7]), bits(got))
    assert np.array_equal(bits(fb.flux_batch(pcm)), bits(fb.flux_apply(rows)))     # lag defaults to 1 in both
