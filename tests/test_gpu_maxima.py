"""sgx_maxima_batch / sgx_maxima_mags: the K strongest spectral maxima per frame, pair and side (include/sgx.h), through the C ABI.

The contract is that the output is a pure function of the row: the stage call equals tests/maxima_reference.py (two masks and a lexsort)
bit for bit on crafted rows of every length class of the kernel; the batch call equals the stage call over the same call's
sgx_stft_batch rows, and the reference, bit for bit on every transform family -- for any split of the call, across the workspace's chunk
seam, at any compute-unit limit, run claim and stream.  Every output buffer is NaN before the call and sits between guard words.

The truth case of the issue asks for a floor of A2 / 2.  A sinusoid of amplitude A at a bin centre has the level A * S1 / W, and the Hann
window has S1 / W = 1 / 2 to rounding, so that floor EQUALS the second sinusoid's level: whether it passes m >= floor is a matter of the
last bit.  The test keeps the literal floor for what it can decide (record 0, its level, every other slot but record 1 zero) and holds
both records and the empty slots under a floor of A2 / 4 as well, which asks more of the empty slots."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_signals as es
import maxima_reference as ref
import stream_cases
from conftest import REL_TOL
from spectrogram_rs_amd import SpectrogramEngine, _lib

pytestmark = pytest.mark.gpu

SR = 48000.0
KS = (1, 2, 5, 64)
GUARD = 64                            # floats before and after every output: 256 bytes, so the output stays 16-byte aligned
WORKSPACE_BYTES = 192 << 20           # include/sgx.h: the bounded workspace
TILE = 2048                           # sgx_maxima.hip: elements of a row one pass of the kernel holds


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def vp(t):
    return C.c_void_p(t.data_ptr())


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


def stage(eng, rows, k, floor=0.0):
    """sgx_maxima_mags over float32 rows [columns][pairs][M][2] on the device -> [columns][pairs][2][k][4], guards checked"""
    import torch

    eng.use_current_stream()
    n = rows.numel() // (eng.pairs * eng.M * 2)
    g = Guarded(eng, n * eng.pairs * 2 * k * 4)
    eng._check(eng._lib.sgx_maxima_mags(eng._ctx, vp(rows), n, C.c_uint32(k), C.c_float(floor), vp(g.out)))
    torch.cuda.current_stream().synchronize()
    assert g.guards_untouched(), "sgx_maxima_mags wrote outside its output"
    return g.out.view(n, eng.pairs, 2, k, 4)


def batch(eng, pcm, k, floor=0.0, first_frame=0, max_frames=None):
    """sgx_maxima_batch -> [frames][pairs][2][k][4], *n_out and the guards checked"""
    import torch

    eng.use_current_stream()
    n_samples = pcm.numel() // eng.channels
    n = max(eng.num_frames(n_samples) - first_frame, 0)
    if max_frames is not None:
        n = min(n, max_frames)
    g = Guarded(eng, n * eng.pairs * 2 * k * 4)
    got = C.c_size_t(7)
    eng._check(eng._lib.sgx_maxima_batch(eng._ctx, vp(pcm), n_samples, first_frame, 2 ** 40 if max_frames is None else max_frames,
                                         C.c_uint32(k), C.c_float(floor), vp(g.out), C.byref(got)))
    torch.cuda.current_stream().synchronize()
    assert got.value == n
    assert g.guards_untouched(), "sgx_maxima_batch wrote outside its output"
    return g.out.view(n, eng.pairs, 2, k, 4)


# ---- 1: the stage call on crafted rows ----------------------------------------------------------------------------------------------------
def seam_rows(M, rng):
    """rows that put the definition's edge cases on the kernel's own seams: the two ends of a wave (64 elements) and of a pass (TILE)"""
    j = np.arange(M)
    h = rng.random(M) + 0.5
    rows = {
        "last_lane": np.where(j % 64 == 63, h, 0.0),
        "first_lane": np.where(j % 64 == 0, h, 0.0),
        "plateau_over_lanes": np.where((j % 64 == 63) | (j % 64 == 0), np.repeat(rng.random(M // 64 + 2), 64)[32:32 + M] + 0.5, 0.0),
        "tie_per_pass": np.where(j % TILE == 7, 1.0, 0.0),                        # one equal candidate in every pass
        "rising_peaks": np.where(j % 16 == 5, (j + 1.0) / M, 0.0),                # the strongest in the last pass, every pass replaces
        "falling_peaks": np.where(j % 16 == 5, (M - j + 0.0) / M, 0.0),           # ... and none does
        "pass_ends": np.where((j % TILE == TILE - 1) | (j % TILE == 0), h, rng.random(M) * 0.25),
    }
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in rows.items()}


STAGE_WINDOWS = {   # M: engine keyword arguments (two pairs: the pair stride)
    3: dict(window_samples=4, hop_samples=1, channels=4),
    5: dict(window_samples=6, hop_samples=2, channels=4),
    255: dict(window_samples=256, hop_samples=64, channels=4),
    256: dict(window_samples=257, hop_samples=64, channels=4),
    257: dict(window_samples=258, hop_samples=64, channels=4),
    2047: dict(window_samples=2048, hop_samples=256, channels=4),
    8191: dict(window_samples=8192, hop_samples=512, channels=4),
    19199: dict(window_samples=19200, hop_samples=4800, channels=4, large_transforms=True),
}


@pytest.mark.parametrize("M", sorted(STAGE_WINDOWS))
def test_stage_on_crafted_rows(M):
    import torch

    eng = SpectrogramEngine(SR, device=0, **STAGE_WINDOWS[M])
    assert eng.M == M and eng.pairs == 2
    if M == 19199:
        assert eng.info.stft_kernel == 11 and M > TILE
    rng = np.random.default_rng(M)
    crafted = dict(ref.crafted_rows(M, rng), **seam_rows(M, rng))
    names = sorted(crafted)
    n = len(names)
    # column c: pair 0 holds (row c, row c + 1), pair 1 (row c + 2, row c + 3): every row meets both sides and both pairs
    rows = np.stack([np.stack([np.stack([crafted[names[(c + 2 * p + s) % n]] for s in range(2)], -1) for p in range(2)]) for c in range(n)])
    assert rows.shape == (n, 2, M, 2)
    dev = torch.from_numpy(rows).to(eng.device)
    floors = [0.0, 0.25, float(np.nextafter(np.float32(0.25), np.float32(1.0)))]      # "constant" and "quantised" hold 0.25 itself
    for k in KS:
        for floor in floors:
            got = stage(eng, dev, k, floor)
            want = ref.maxima(rows, k, floor)
            if not np.array_equal(bits(got), np_bits(want)):
                g = got.cpu().numpy()
                bad = [(names[(c + 2 * p + s) % n], c, p, s) for c in range(n) for p in range(2) for s in range(2)
                       if not np.array_equal(np_bits(g[c, p, s]), np_bits(want[c, p, s]))]
                raise AssertionError(f"M {M}, K {k}, floor {floor}: not the reference's bits on {bad[:6]}")
    # the cases the rows were made for did occur
    want = ref.maxima(rows, 64, 0.0)
    filled = (want[..., 0] != 0).sum(-1)
    assert filled.min() == 0 and (M < 8 or filled.max() >= min(64, (M - 2) // 2) // 2)   # empty rows, and rows with more candidates than K
    if M >= 5:
        c = names.index("strongest_at_1")
        assert want[c, 0, 0, 0, 0] == 2.0
        c = names.index("strongest_at_last_interior")
        assert want[c, 0, 0, 0, 0] == float(M - 1)
        c = names.index("ends_larger")
        bins = want[c, 0, 0, :, 0]
        assert 1.0 not in bins and float(M) not in bins and 2.0 not in bins and float(M - 1) not in bins
        c = names.index("ends_as_neighbours")                                     # (9, 10, ..., 10, 9): the ends' values as neighbours
        assert want[c, 0, 0, 0, :3].tolist() == [2.0, 9.0, 10.0] and want[c, 0, 0, 1, 0] == float(M - 1) and want[c, 0, 0, 1, 3] == 9.0
        assert 1.0 not in want[c, 0, 0, :, 0] and float(M) not in want[c, 0, 0, :, 0]
    eng.close()


# ---- 2: the batch call on one context per transform family ----------------------------------------------------------------------------------
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
    """the engine's white noise at 0.1 plus two tones per channel, off the bin centres"""
    import torch

    n = eng.W + (frames - 1) * eng.H
    t = torch.arange(n, dtype=torch.float64, device=eng.device)
    pcm = 0.1 * eng.white_noise(n, seed=seed).view(n, eng.channels)
    for c in range(eng.channels):
        for amp, frac in ((0.5, 0.123 + 0.01 * c), (0.3, 0.371 - 0.01 * c)):
            pcm[:, c] += (amp * torch.cos(np.pi * frac * t)).float()
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
    pcm = tones_in_noise(eng, frames, seed=0x3A71 + len(label))
    rows = eng.stft_batch(pcm)
    torch.cuda.synchronize()
    host = rows.cpu().numpy()
    host.setflags(write=False)
    return eng, pcm, rows, host


@pytest.mark.parametrize("label", sorted(FAMILY_ROUTES))
def test_batch_on_every_family(label):
    eng, pcm, rows, host = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    floor = float(np.float32(np.median(host)))
    for k, fl in ((5, 0.0), (64, floor), (1, 0.0)):
        got = batch(eng, pcm, k, fl)
        assert got.shape == (frames, eng.pairs, 2, k, 4)
        staged = stage(eng, rows, k, fl)
        assert np.array_equal(bits(got), bits(staged)), f"{label}/K {k}: the batch call differs from the stage call over its own rows"
        assert np.array_equal(bits(got), np_bits(ref.maxima(host, k, fl))), f"{label}/K {k}: not the reference's bits"
    # the two tones are the two strongest maxima of every frame and side
    top = batch(eng, pcm, 2).cpu().numpy()
    for c in range(min(eng.channels, 2)):
        centres = sorted(2.0 * eng.W * f / 2.0 for f in (0.123 + 0.01 * c, 0.371 - 0.01 * c))
        found = np.sort(top[:, 0, c, :, 0], axis=-1)
        assert (np.abs(found - np.array(centres)) <= 1.0).all(), f"{label}: side {c} does not find its tones"
    if eng.channels == 1 and "paired_frames" not in es.ROUTE[FAMILY_ROUTES[label][0]].flags:
        assert np.array_equal(np_bits(top[:, :, 0]), np_bits(top[:, :, 1])), f"{label}: a mono stream does not hold the same records twice"


# ---- 3: splits and seams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "w4800", "w16384", "large"])
def test_split_calls_equal_one_call(label):
    eng, pcm, _, _ = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    k = 5
    full = batch(eng, pcm, k)
    cut = frames // 2 if (frames // 2) % 2 else frames // 2 + 1                     # an odd frame
    parts = [batch(eng, pcm, k, max_frames=cut), batch(eng, pcm, k, first_frame=cut)]
    assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(full)), f"{label}: split at frame {cut}"
    if frames >= 8:
        first = 3
        cut = first + (frames - first) // 2
        cut += 1 - cut % 2
        parts = [batch(eng, pcm, k, first_frame=first, max_frames=cut - first), batch(eng, pcm, k, first_frame=cut)]
        assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(full[first:])), f"{label}: frames {first} .. split at {cut}"


def test_workspace_chunk_seam_at_w8192_ch8():
    """W 8192 with 8 channels: a frame's rows are 262 112 bytes, 768 frames fit the workspace; 800 frames cross the seam"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=8192, hop_samples=64, channels=8)
    frames = 800
    per_chunk = WORKSPACE_BYTES // (eng.pairs * eng.M * 8)
    assert 1 < per_chunk < frames - 8
    pcm = tones_in_noise(eng, frames, seed=99)
    rows = eng.stft_batch(pcm)
    k = 8
    got = batch(eng, pcm, k)
    staged = stage(eng, rows, k)
    assert torch.equal(got.view(torch.int32), staged.view(torch.int32)), "the batch call across the chunk seam differs from the stage call"
    lo, hi = per_chunk - 2, per_chunk + 2                                         # the reference on the frames either side of the seam
    want = ref.maxima(rows[lo:hi].cpu().numpy(), k)
    assert np.array_equal(bits(got[lo:hi]), np_bits(want))
    parts = [batch(eng, pcm, k, max_frames=per_chunk + 1), batch(eng, pcm, k, first_frame=per_chunk + 1)]
    assert torch.equal(torch.cat(parts).view(torch.int32), got.view(torch.int32))
    eng.close()


# ---- 4: independence of compute-unit limit, run claim and stream ---------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "wg4096_ch4", "w4800", "w16384"])
def test_cu_limits_and_streams(label):
    import torch

    eng, pcm, _, _ = family_context(label)
    k = 5
    try:
        expect = bits(batch(eng, pcm, k))
        for limit in (1, 3, 0):
            eng.set_cu_limit(limit)
            assert np.array_equal(bits(batch(eng, pcm, k)), expect), f"{label}: {limit} compute units"
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                                # (batch() binds the engine to torch's current stream)
            other = batch(eng, pcm, k)
        s.synchronize()
        assert np.array_equal(bits(other), expect), f"{label}: a non-default stream"
    finally:
        eng.set_cu_limit(0)
        eng.use_current_stream()
    torch.cuda.synchronize()


def test_run_claims_on_the_mono_w2048_context():
    eng, pcm, _, _ = family_context("wg4096_real_h256")
    k = 5
    try:
        eng.set_run_claim(16, 0)
        static = bits(batch(eng, pcm, k))
        eng.set_run_claim(4, 8)
        claimed = bits(batch(eng, pcm, k))
    finally:
        eng.set_run_claim(0, 0)
    assert np.array_equal(static, claimed)
    assert np.array_equal(static, bits(batch(eng, pcm, k)))


# ---- 5: truth -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(window_samples=2048, hop_samples=256, channels=1), dict(window_samples=2048, hop_samples=256, channels=2),
                                dict(window_samples=2400, hop_samples=93, channels=2), dict(window_samples=64, hop_samples=16, channels=2),
                                dict(window_samples=8192, hop_samples=512, channels=2)], ids=lambda kw: f"w{kw['window_samples']}_ch{kw['channels']}")
def test_two_sinusoids_at_bin_centres(kw):
    import torch

    eng = SpectrogramEngine(SR, device=0, **kw)
    W, frames, k = eng.W, 12, 6
    a1, a2 = 0.5, 0.25
    k1, k2 = W // 2, W // 4                                                       # bins of the 2W-point transform: cos(pi n / 2), cos(pi n / 4)
    n = W + (frames - 1) * eng.H
    t = np.arange(n)
    tone = (a1 * np.cos(np.pi * k1 * t / W) + a2 * np.cos(np.pi * k2 * t / W)).astype(np.float32)
    pcm = torch.from_numpy(np.repeat(tone[:, None], eng.channels, 1).reshape(-1).copy()).to(eng.device)
    s1_w = float(eng.window().astype(np.float64).sum()) / W
    levels = (a1 * s1_w, a2 * s1_w)
    # the issue's floor, A2 / 2: the second sinusoid's own level to rounding (module docstring), so record 1 is that bin or empty
    got = batch(eng, pcm, k, a2 / 2).cpu().numpy().astype(np.float64)
    print(f"level 2 = {levels[1]!r}, floor A2 / 2 = {a2 / 2!r}, record 1 bins under it: {sorted(set(got[..., 1, 0].reshape(-1)))}")
    assert (got[..., 0, 0] == k1).all()
    worst = float(np.abs(got[..., 0, 2] - levels[0]).max() / (REL_TOL * levels[0]))
    print(f"floor A2 / 2: worst |centre 1 - A1 S1 / W| / (REL_TOL level) = {worst:.3f}")
    assert worst <= 1.0
    assert np.isin(got[..., 1, 0], (0.0, float(k2))).all() and not got[..., 2:, :].any()
    # a floor of A2 / 4 decides both records; the empty slots are empty under the lower floor too
    got = batch(eng, pcm, k, a2 / 4).cpu().numpy().astype(np.float64)
    assert (got[..., 0, 0] == k1).all() and (got[..., 1, 0] == k2).all()
    for r, level in enumerate(levels):
        worst = float(np.abs(got[..., r, 2] - level).max() / (REL_TOL * level))
        print(f"floor A2 / 4: worst |centre {r + 1} - A S1 / W| / (REL_TOL level) = {worst:.3f}")
        assert worst <= 1.0, f"record {r}"
        assert (got[..., r, 1] < got[..., r, 2]).all() and (got[..., r, 3] <= got[..., r, 2]).all()
    assert not got[..., 2:, :].any(), "slots beyond the two sinusoids are not empty"
    eng.close()


# ---- 6: far offsets -------------------------------------------------------------------------------------------------------------------------
def test_output_beyond_4_gib():
    """W 4 is the smallest window the library takes (the generic kernel's 8-point transform): M = 3, one interior bin.  K = 64 makes a
    column 2 048 bytes, so 2^21 + 3 columns end beyond 2^32 bytes of d_max"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=4, hop_samples=1, channels=2)
    assert eng.info.stft_kernel == 0 and eng.M == 3
    k, cols = 64, (1 << 21) + 3
    assert cols * 2 * k * 4 * 4 > 1 << 32
    rows = torch.zeros((cols, 1, 3, 2), dtype=torch.float32, device=eng.device)
    edge = np.random.default_rng(4).random((6, 1, 3, 2)).astype(np.float32)
    edge[:, :, 1] += 1.0                                                          # the interior bin is a maximum on both sides
    edge[1, 0, 1, 0] = 0.0                                                        # ... but for one column's left side
    rows[:3] = torch.from_numpy(edge[:3]).to(eng.device)
    rows[-3:] = torch.from_numpy(edge[3:]).to(eng.device)
    g = Guarded(eng, cols * 2 * k * 4)
    eng._check(eng._lib.sgx_maxima_mags(eng._ctx, vp(rows), cols, C.c_uint32(k), C.c_float(0.0), vp(g.out)))
    torch.cuda.synchronize()
    out = g.out.view(cols, 1, 2, k, 4)
    assert np.array_equal(bits(out[:3]), np_bits(ref.maxima(edge[:3], k)))
    assert np.array_equal(bits(out[-3:]), np_bits(ref.maxima(edge[3:], k)))
    assert not out[3:-3].any().item(), "the all-zero columns between them are not empty records"
    now_head, now_tail = bits(g.buf[:GUARD]), bits(g.buf[-GUARD:])
    assert np.array_equal(now_head, g.stale[:GUARD]) and np.array_equal(now_tail, g.stale[-GUARD:])
    del g, out, rows
    eng.close()
    torch.cuda.empty_cache()


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch

    eng, pcm, rows, _ = family_context("wg4096_lr")
    frames = FAMILY_ROUTES["wg4096_lr"][2]
    n = pcm.numel() // eng.channels
    lib, bad = eng._lib, _lib.SGX_ERR_INVALID_ARG
    g = Guarded(eng, frames * eng.pairs * 2 * 64 * 4)
    out, off = vp(g.out), C.c_void_p(g.out.data_ptr() + 4)
    u, f = C.c_uint32, C.c_float
    got = C.c_size_t(7)

    def batch_call(ctx=eng._ctx, d_pcm=vp(pcm), k=5, floor=0.0, d_max=out):
        return lib.sgx_maxima_batch(ctx, d_pcm, n, 0, 1000, u(k), f(floor), d_max, C.byref(got))

    def stage_call(ctx=eng._ctx, d_mags=vp(rows), k=5, floor=0.0, d_max=out):
        return lib.sgx_maxima_mags(ctx, d_mags, frames, u(k), f(floor), d_max)

    for call, who in ((batch_call, b"sgx_maxima_batch"), (stage_call, b"sgx_maxima_mags")):
        for kw in (dict(k=0), dict(k=65), dict(floor=-1e-30), dict(floor=float("nan")), dict(floor=float("inf")), dict(d_max=off),
                   dict(d_max=None), {"d_pcm" if call is batch_call else "d_mags": None}):
            got.value = 7
            assert call(**kw) == bad, (who, kw)
            assert who in lib.sgx_last_error(eng._ctx), (who, kw, lib.sgx_last_error(eng._ctx))
            assert call is stage_call or got.value == 0
        assert call(ctx=None) == bad
    assert b"aligned" in (batch_call(d_max=off), lib.sgx_last_error(eng._ctx))[1]
    # not errors: too few samples, no frame in range, no columns, a null n_out
    got.value = 7
    assert lib.sgx_maxima_batch(eng._ctx, vp(pcm), eng.W - 1, 0, 10, u(5), f(0.0), out, C.byref(got)) == 0 and got.value == 0
    got.value = 7
    assert lib.sgx_maxima_batch(eng._ctx, vp(pcm), n, frames, 10, u(5), f(0.0), out, C.byref(got)) == 0 and got.value == 0
    assert lib.sgx_maxima_mags(eng._ctx, vp(rows), 0, u(5), f(0.0), out) == 0
    torch.cuda.synchronize()
    assert g.untouched(), "a refused or empty call wrote to its buffer"
    assert lib.sgx_maxima_batch(eng._ctx, vp(pcm), n, 0, 1000, u(5), f(0.0), out, None) == 0
    torch.cuda.synchronize()
    assert g.guards_untouched() and np.array_equal(bits(g.out[:frames * eng.pairs * 2 * 5 * 4]), bits(batch(eng, pcm, 5)))


def test_python_methods():
    eng, pcm, rows, host = family_context("wg4096_ch4")
    got = eng.maxima_batch(pcm, 3, floor=0.01, first_frame=2, max_frames=5)
    assert got.shape == (5, eng.pairs, 2, 3, 4)
    assert np.array_equal(bits(got), np_bits(ref.maxima(host[2:7], 3, 0.01)))
    assert np.array_equal(bits(eng.maxima_mags(rows[2:7].contiguous(), 3, floor=0.01)), bits(got))
