"""sgx_rolloff_batch / sgx_rolloff_mags: where the running sum of a frame's row crosses shares of its total (include/sgx.h), through the
C ABI.

The contract is that the output is a pure function of the row: the stage call equals tests/rolloff_reference.py (two np.cumsum calls and
one add) bit for bit on crafted rows either side of a segment (32 elements), of a tile of 64 segments and over several tiles; the batch
call equals the stage call over the same call's sgx_stft_batch rows, and the reference, bit for bit on every transform family -- for any
split of the call, across the workspace's chunk seam, at any compute-unit limit, run claim and stream.  Every output buffer is NaN before
the call and sits between guard words (the helpers and the family contexts are those of tests/test_gpu_maxima.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import rolloff_reference as ref
from conftest import REL_TOL
from spectrogram_rs_amd import SpectrogramEngine, _lib
from test_gpu_maxima import FAMILY_ROUTES, GUARD, SR, WORKSPACE_BYTES, Guarded, bits, family_context, np_bits, tones_in_noise, vp
import edge_signals as es

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EIGHT = (0.005, 0.05, 0.25, 0.5, 0.75, 0.85, 0.95, 0.995)
SHARES = ((0.5,), (1.0,), (0.85, 0.05, 0.85, 2.0 ** -20), EIGHT)
assert GUARD % 4 == 0                 # the output stays 16-byte aligned behind the guard


def shares(p):
    return (C.c_float * len(p))(*p), C.c_uint32(len(p))


def stage(eng, rows, power, p):
    """sgx_rolloff_mags over float32 rows [columns][pairs][M][2] on the device -> [columns][pairs][2][n_p][4], guards checked"""
    import torch

    eng.use_current_stream()
    n = rows.numel() // (eng.pairs * eng.M * 2)
    g = Guarded(eng, n * eng.pairs * 2 * len(p) * 4)
    h_p, n_p = shares(p)
    eng._check(eng._lib.sgx_rolloff_mags(eng._ctx, vp(rows), n, C.c_uint32(power), h_p, n_p, vp(g.out)))
    torch.cuda.current_stream().synchronize()
    assert g.guards_untouched(), "sgx_rolloff_mags wrote outside its output"
    return g.out.view(n, eng.pairs, 2, len(p), 4)


def batch(eng, pcm, power, p, first_frame=0, max_frames=None):
    """sgx_rolloff_batch -> [frames][pairs][2][n_p][4], *n_out and the guards checked"""
    import torch

    eng.use_current_stream()
    n_samples = pcm.numel() // eng.channels
    n = max(eng.num_frames(n_samples) - first_frame, 0)
    if max_frames is not None:
        n = min(n, max_frames)
    g = Guarded(eng, n * eng.pairs * 2 * len(p) * 4)
    got = C.c_size_t(7)
    h_p, n_p = shares(p)
    eng._check(eng._lib.sgx_rolloff_batch(eng._ctx, vp(pcm), n_samples, first_frame, 2 ** 40 if max_frames is None else max_frames,
                                          C.c_uint32(power), h_p, n_p, vp(g.out), C.byref(got)))
    torch.cuda.current_stream().synchronize()
    assert got.value == n
    assert g.guards_untouched(), "sgx_rolloff_batch wrote outside its output"
    return g.out.view(n, eng.pairs, 2, len(p), 4)


# ---- 1: the stage call on crafted rows ----------------------------------------------------------------------------------------------------
STAGE_WINDOWS = {   # M: engine keyword arguments (two pairs: the pair stride)
    3: dict(window_samples=4, hop_samples=1, channels=4),
    31: dict(window_samples=32, hop_samples=8, channels=4),
    32: dict(window_samples=33, hop_samples=8, channels=4),
    33: dict(window_samples=34, hop_samples=8, channels=4),
    2047: dict(window_samples=2048, hop_samples=256, channels=4),
    2048: dict(window_samples=2049, hop_samples=256, channels=4),
    2049: dict(window_samples=2050, hop_samples=256, channels=4),
    8191: dict(window_samples=8192, hop_samples=512, channels=4),
    19199: dict(window_samples=19200, hop_samples=4800, channels=4, large_transforms=True),
}


def test_stage_on_crafted_rows():
    for M in sorted(STAGE_WINDOWS):
        stage_on_crafted_rows(M)


def stage_on_crafted_rows(M):
    import torch

    eng = SpectrogramEngine(SR, device=0, **STAGE_WINDOWS[M])
    assert eng.M == M and eng.pairs == 2
    crafted = ref.crafted_rows(M, np.random.default_rng(M))
    names = sorted(crafted)
    n = len(names)
    # column c: pair 0 holds (row c, row c + 1), pair 1 (row c + 2, row c + 3): every row meets both sides and both pairs
    which = np.array([[[(c + 2 * p + s) % n for s in range(2)] for p in range(2)] for c in range(n)])
    rows = np.stack([np.stack([np.stack([crafted[names[which[c, p, s]]] for s in range(2)], -1) for p in range(2)]) for c in range(n)])
    assert rows.shape == (n, 2, M, 2)
    nan = which == names.index("nan_in_the_middle")
    dev = torch.from_numpy(rows).to(eng.device)
    for power in (1, 2):
        for p in SHARES:
            got = stage(eng, dev, power, p).cpu().numpy()
            want = ref.rolloff(rows, power, p)
            # the NaN row: (0, 0, 0, NaN) in its own records, whatever the NaN's bits
            assert np.isnan(want[nan][..., 3]).all() and not want[nan][..., :3].any()
            assert np.isnan(got[nan][..., 3]).all() and not np_bits(got[nan][..., :3]).any(), f"M {M}, power {power}, p {p}: the NaN row"
            if not np.array_equal(np_bits(got[~nan]), np_bits(want[~nan])):
                bad = [(names[which[c, q, s]], c, q, s, got[c, q, s].tolist(), want[c, q, s].tolist()) for c in range(n) for q in range(2)
                       for s in range(2) if not nan[c, q, s] and not np.array_equal(np_bits(got[c, q, s]), np_bits(want[c, q, s]))]
                raise AssertionError(f"M {M}, power {power}, p {p}: not the reference's bits on {bad[:3]}")
    # the cases the rows were made for did occur
    want = ref.rolloff(rows, 1, (0.5, 1.0))
    at = {name: want[names.index(name), 0, 0] for name in names}
    assert at["zero"].tolist() == [[0, 0, 0, 0]] * 2 and at["only_first"][:, 0].tolist() == [1, 1] and at["only_last"][:, 0].tolist() == [M, M]
    assert at["only_31"][:, 0].tolist() == [min(32, M)] * 2 and at["only_32"][:, 0].tolist() == [min(33, M)] * 2
    assert at["huge_first"][:, 0].tolist() == [1, 1]
    if M == 2048:
        assert at["ones"].tolist() == [[1024, 1023, 1024, 2048], [2048, 2047, 2048, 2048]]   # thr = c[1023] exactly: >= decides the tie
    eng.close()


# ---- 2: the batch call on one context per transform family ----------------------------------------------------------------------------------
BATCH_CASES = ((2, (0.85,)), (1, (0.5, 0.95, 0.05)), (2, EIGHT))


def test_batch_on_every_family():
    for label in sorted(FAMILY_ROUTES):
        batch_on_family(label)


def batch_on_family(label):
    eng, pcm, rows, host = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    for power, p in BATCH_CASES:
        got = batch(eng, pcm, power, p)
        assert got.shape == (frames, eng.pairs, 2, len(p), 4)
        staged = stage(eng, rows, power, p)
        assert np.array_equal(bits(got), bits(staged)), f"{label}/power {power}/{p}: the batch call differs from the stage call over its own rows"
        assert np.array_equal(bits(got), np_bits(ref.rolloff(host, power, p))), f"{label}/power {power}/{p}: not the reference's bits"
        if eng.channels == 1 and "paired_frames" not in es.ROUTE[FAMILY_ROUTES[label][0]].flags:
            assert np.array_equal(bits(got[:, :, 0]), bits(got[:, :, 1])), f"{label}: a mono stream does not hold the same records twice"
        assert (got[..., 0] >= 1).all().item() and (got[..., 3] > 0).all().item()


# ---- 3: seams and independence -----------------------------------------------------------------------------------------------------------
P3 = (0.5, 0.95, 0.05)


def test_seams_and_independence():
    for label in ("wg4096_real_h256", "wg4096_lr", "w4800", "w16384", "large"):
        split_calls_equal_one_call(label)
    workspace_chunk_seam_at_w8192_ch8()
    for label in ("wg4096_real_h256", "wg4096_lr", "wg4096_ch4", "w4800", "w16384"):
        cu_limits_and_streams(label)
    run_claims_on_the_mono_w2048_context()
    six_channels()


def split_calls_equal_one_call(label):
    eng, pcm, _, _ = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    full = batch(eng, pcm, 2, P3)
    cut = frames // 2 if (frames // 2) % 2 else frames // 2 + 1                     # an odd frame
    parts = [batch(eng, pcm, 2, P3, max_frames=cut), batch(eng, pcm, 2, P3, first_frame=cut)]
    assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(full)), f"{label}: split at frame {cut}"
    first = 3
    cut = first + (frames - first) // 2
    cut += 1 - cut % 2
    parts = [batch(eng, pcm, 2, P3, first_frame=first, max_frames=cut - first), batch(eng, pcm, 2, P3, first_frame=cut)]
    assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(full[first:])), f"{label}: frames {first} .. split at {cut}"


def workspace_chunk_seam_at_w8192_ch8():
    """W 8192 with 8 channels: a frame's rows are 262 112 bytes, 768 frames fit the workspace; 800 frames cross the seam"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=8192, hop_samples=64, channels=8)
    frames = 800
    per_chunk = WORKSPACE_BYTES // (eng.pairs * eng.M * 8)
    assert per_chunk == 768
    pcm = tones_in_noise(eng, frames, seed=99)
    rows = eng.stft_batch(pcm)
    got = batch(eng, pcm, 2, P3)
    staged = stage(eng, rows, 2, P3)
    assert torch.equal(got.view(torch.int32), staged.view(torch.int32)), "the batch call across the chunk seam differs from the stage call"
    lo, hi = per_chunk - 2, per_chunk + 2                                         # the reference on the frames either side of the seam
    assert np.array_equal(bits(got[lo:hi]), np_bits(ref.rolloff(rows[lo:hi].cpu().numpy(), 2, P3)))
    parts = [batch(eng, pcm, 2, P3, max_frames=per_chunk + 1), batch(eng, pcm, 2, P3, first_frame=per_chunk + 1)]
    assert torch.equal(torch.cat(parts).view(torch.int32), got.view(torch.int32))
    eng.close()


def cu_limits_and_streams(label):
    import torch

    eng, pcm, _, _ = family_context(label)
    try:
        expect = bits(batch(eng, pcm, 2, P3))
        for limit in (1, 3, 0):
            eng.set_cu_limit(limit)
            assert np.array_equal(bits(batch(eng, pcm, 2, P3)), expect), f"{label}: {limit} compute units"
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                                # (batch() binds the engine to torch's current stream)
            other = batch(eng, pcm, 2, P3)
        s.synchronize()
        assert np.array_equal(bits(other), expect), f"{label}: a non-default stream"
    finally:
        eng.set_cu_limit(0)
        eng.use_current_stream()
    torch.cuda.synchronize()


def run_claims_on_the_mono_w2048_context():
    eng, pcm, _, _ = family_context("wg4096_real_h256")
    try:
        eng.set_run_claim(16, 0)
        static = bits(batch(eng, pcm, 2, P3))
        eng.set_run_claim(4, 8)
        claimed = bits(batch(eng, pcm, 2, P3))
    finally:
        eng.set_run_claim(0, 0)
    assert np.array_equal(static, claimed)
    assert np.array_equal(static, bits(batch(eng, pcm, 2, P3)))


def six_channels():
    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=256, channels=6)
    assert eng.pairs == 3
    pcm = tones_in_noise(eng, 9, seed=6)
    rows = eng.stft_batch(pcm)
    for power, p in BATCH_CASES:
        got = batch(eng, pcm, power, p)
        assert got.shape == (9, 3, 2, len(p), 4)
        assert np.array_equal(bits(got), bits(stage(eng, rows, power, p)))
        assert np.array_equal(bits(got), np_bits(ref.rolloff(rows.cpu().numpy(), power, p)))
    assert len({bits(got[:, q]).tobytes() for q in range(3)}) == 3                # the pairs hold different records
    eng.close()


# ---- 4: truth -------------------------------------------------------------------------------------------------------------------------------
def test_truth():
    for W, H in ((64, 16), (2048, 256), (2400, 93), (8192, 512)):
        two_sinusoids_at_bin_centres(W, H)
    for label in sorted(FAMILY_ROUTES):
        float64_bracket_on_the_family_rows(label)


def two_sinusoids_at_bin_centres(W, H):
    """Amplitudes 0.5 at bin W / 4 and 0.25 at bin W / 2 of the 2W-point transform: at power 2 the energy shares are 0.8 / 0.2, each
    tone's lobe symmetric about its centre bin, so half of the first share is reached in k1 and nine tenths of the total in k2"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=W, hop_samples=H, channels=2)
    frames = 12
    k1, k2 = W // 4, W // 2
    n = W + (frames - 1) * H
    t = np.arange(n)
    tone = (0.5 * np.cos(np.pi * k1 * t / W) + 0.25 * np.cos(np.pi * k2 * t / W)).astype(np.float32)
    pcm = torch.from_numpy(np.repeat(tone[:, None], 2, 1).reshape(-1).copy()).to(eng.device)
    got = batch(eng, pcm, 2, (0.5, 0.9)).cpu().numpy().astype(np.float64)
    assert (got[..., 0, 0] == k1).all(), sorted(set(got[..., 0, 0].reshape(-1)))
    assert (got[..., 1, 0] == k2).all(), sorted(set(got[..., 1, 0].reshape(-1)))
    rows = eng.stft_batch(pcm).cpu().numpy().astype(np.float64)                   # [frames][1][M][2]
    t64 = (rows ** 2).sum(-2)                                                     # [frames][1][2]
    worst = float((np.abs(got[..., 3] - t64[..., None]) / (REL_TOL * t64[..., None])).max())
    print(f"W {W}: worst |T - T64| / (REL_TOL T64) = {worst:.4f}")
    assert worst <= 1.0
    assert (got[..., 1] < got[..., 2]).all() and (got[..., 2] <= got[..., 3]).all()
    eng.close()


def float64_bracket_on_the_family_rows(label):
    """The crossing the call names is the float64 crossing to within the arithmetic bound of the definition (include/sgx.h): with
    delta = (32 + ceil(M / 32) + 3) * 2^-24, C64[j*] >= (p - 2 delta) T64 and (j* = 0 or C64[j* - 1] < (p + 2 delta) T64)"""
    eng, pcm, _, host = family_context(label)
    delta = (32 + math.ceil(eng.M / 32) + 3) * U
    for power, p in BATCH_CASES:
        got = batch(eng, pcm, power, p).cpu().numpy()
        c64 = np.moveaxis(np.cumsum(host.astype(np.float64) ** power, axis=-2), -1, -2)   # [frames][pairs][2][M]
        t64 = c64[..., -1]
        worst = -np.inf
        for i, share in enumerate(p):
            j = got[..., i, 0].astype(np.int64) - 1
            assert (j >= 0).all()
            at = np.take_along_axis(c64, j[..., None], -1)[..., 0]
            below = np.take_along_axis(c64, np.maximum(j - 1, 0)[..., None], -1)[..., 0]
            share = float(np.float32(share))
            lower = ((share - 2 * delta) * t64 - at) / (delta * t64)              # <= 0 asked
            upper = np.where(j > 0, (below - (share + 2 * delta) * t64) / (delta * t64), -np.inf)   # < 0 asked
            worst = max(worst, float(lower.max()), float(upper.max()))
            assert (lower <= 0).all() and (upper < 0).all(), f"{label}/power {power}/p {share}"
        print(f"{label}/power {power}: the bracket's worst margin is {worst:.3f} delta of the total short of failing (negative: holds)")


# ---- 5: far offsets -------------------------------------------------------------------------------------------------------------------------
def test_rows_beyond_4_gib():
    """W 2048 mono: a row is 16 376 bytes, so 262 277 rows end beyond 2^32 bytes of d_mags"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=256, channels=1)
    assert eng.M == 2047 and eng.pairs == 1
    cols = (1 << 32) // (eng.M * 8) + 4
    assert (cols - 3) * eng.M * 8 > 1 << 32
    rows = torch.zeros((cols, 1, eng.M, 2), dtype=torch.float32, device=eng.device)
    edge = np.random.default_rng(5).random((6, 1, eng.M, 2)).astype(np.float32)
    rows[:3] = torch.from_numpy(edge[:3]).to(eng.device)
    rows[-3:] = torch.from_numpy(edge[3:]).to(eng.device)
    p = (0.85, 0.05, 0.5)
    out = stage(eng, rows, 2, p)
    assert np.array_equal(bits(out[:3]), np_bits(ref.rolloff(edge[:3], 2, p)))
    assert np.array_equal(bits(out[-3:]), np_bits(ref.rolloff(edge[3:], 2, p)))
    assert not out[3:-3].view(torch.int32).any().item(), "the all-zero rows between them are not (0, 0, 0, 0)"
    del out, rows
    eng.close()
    torch.cuda.empty_cache()


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch

    eng, pcm, rows, _ = family_context("wg4096_lr")
    frames = FAMILY_ROUTES["wg4096_lr"][2]
    n = pcm.numel() // eng.channels
    lib, bad = eng._lib, _lib.SGX_ERR_INVALID_ARG
    g = Guarded(eng, frames * eng.pairs * 2 * 8 * 4)
    out, off = vp(g.out), C.c_void_p(g.out.data_ptr() + 4)
    got = C.c_size_t(7)
    null_p = C.POINTER(C.c_float)()

    def batch_call(ctx=eng._ctx, d_pcm=vp(pcm), power=2, p=(0.85,), n_p=None, d_out=out):
        h_p = null_p if p is None else (C.c_float * max(len(p), 9))(*p)
        return lib.sgx_rolloff_batch(ctx, d_pcm, n, 0, 1000, C.c_uint32(power), h_p, C.c_uint32(len(p) if n_p is None else n_p), d_out,
                                     C.byref(got))

    def stage_call(ctx=eng._ctx, d_mags=vp(rows), power=2, p=(0.85,), n_p=None, d_out=out):
        h_p = null_p if p is None else (C.c_float * max(len(p), 9))(*p)
        return lib.sgx_rolloff_mags(ctx, d_mags, frames, C.c_uint32(power), h_p, C.c_uint32(len(p) if n_p is None else n_p), d_out)

    above_one = float(np.nextafter(np.float32(1.0), np.float32(2.0)))               # 1.0000001
    for call, who in ((batch_call, b"sgx_rolloff_batch"), (stage_call, b"sgx_rolloff_mags")):
        for kw in (dict(power=0), dict(power=3), dict(n_p=0), dict(p=(0.5,) * 9), dict(p=(0.0,)), dict(p=(0.5, -0.5)), dict(p=(above_one,)),
                   dict(p=(0.5, 0.5, float("nan"))), dict(p=None, n_p=1), dict(d_out=None), dict(d_out=off),
                   {"d_pcm" if call is batch_call else "d_mags": None}):
            got.value = 7
            assert call(**kw) == bad, (who, kw)
            assert who in lib.sgx_last_error(eng._ctx), (who, kw, lib.sgx_last_error(eng._ctx))
            assert call is stage_call or got.value == 0
        assert call(ctx=None) == bad
    assert b"aligned" in (batch_call(d_out=off), lib.sgx_last_error(eng._ctx))[1]
    # not errors: too few samples, no frame in range, no columns, a null n_out
    h_p, n_p = shares((0.85,))
    got.value = 7
    assert lib.sgx_rolloff_batch(eng._ctx, vp(pcm), eng.W - 1, 0, 10, C.c_uint32(2), h_p, n_p, out, C.byref(got)) == 0 and got.value == 0
    got.value = 7
    assert lib.sgx_rolloff_batch(eng._ctx, vp(pcm), n, frames, 10, C.c_uint32(2), h_p, n_p, out, C.byref(got)) == 0 and got.value == 0
    assert lib.sgx_rolloff_mags(eng._ctx, vp(rows), 0, C.c_uint32(2), h_p, n_p, out) == 0
    torch.cuda.synchronize()
    assert g.untouched(), "a refused or empty call wrote to its buffer"
    assert lib.sgx_rolloff_batch(eng._ctx, vp(pcm), n, 0, 1000, C.c_uint32(2), h_p, n_p, out, None) == 0
    torch.cuda.synchronize()
    assert g.guards_untouched() and np.array_equal(bits(g.out[:frames * eng.pairs * 2 * 4]), bits(batch(eng, pcm, 2, (0.85,))))


# ---- 7: the Python methods ------------------------------------------------------------------------------------------------------------------
def test_python_methods():
    eng, pcm, rows, host = family_context("wg4096_ch4")
    got = eng.rolloff_batch(pcm, 2, (0.85, 0.5), first_frame=2, max_frames=5)
    assert got.shape == (5, eng.pairs, 2, 2, 4)
    assert np.array_equal(bits(got), np_bits(ref.rolloff(host[2:7], 2, (0.85, 0.5))))
    assert np.array_equal(bits(eng.rolloff_mags(rows[2:7].contiguous(), 2, (0.85, 0.5))), bits(got))
    assert np.array_equal(bits(eng.rolloff_mags(rows[:1].contiguous(), 1, 0.5)), np_bits(ref.rolloff(host[:1], 1, (0.5,))))
