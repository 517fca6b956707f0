"""sgx_quantile_batch / sgx_quantile_mags: per-bin order statistics over groups of frames (include/sgx.h), through the C ABI.

The output is one of the column's own float32 words, so every comparison is on bit patterns: the stage call equals
tests/quantile_reference.py (key, np.sort along the frame axis, the rank rule, un-key) on crafted rows on both sides of the kernel's
path decision and across its tile; the batch call equals the stage call over the same call's sgx_stft_batch rows, and the reference, on
every transform family -- for any split at a column boundary, across the workspace's range seam, at any compute-unit limit, run claim
and stream.  Every output buffer is NaN before the call and sits between guard words.

The truth case holds the median to conftest.REL_TOL by that tolerance's own rule, |x - truth| <= REL_TOL * max(|truth|, floor * peak);
W 256 is none of the baseline kernels, so the floor is conftest.FLOOR_WIDE, the one "every other window" is held to."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_signals as es
import oracle
import quantile_reference as ref
import stream_cases
from conftest import FLOOR_WIDE, REL_TOL, mags_error
from spectrogram_rs_amd import SpectrogramEngine, _lib

pytestmark = pytest.mark.gpu

SR = 48000.0
GUARD = 64                            # floats before and after every output
TILE = 64                             # sgx_quantile.hpp: kTile, the consecutive elements of a row one workgroup of path A owns
LDS_FRAMES = 512                      # sgx_quantile.hpp: kLdsFrames, the longest column path A selects in LDS
SIZE_MAX = ref.SIZE_MAX
Q1 = (0.5,)
Q5 = (0.0, 0.1, 0.5, 0.9, 1.0)
Q16 = (1.0, 0.9, 0.9, 0.75, 0.5, 0.5, 0.5, 0.3, 0.25, 0.2, 0.1, 0.1, 0.05, 0.01, 0.0, 0.0)    # descending, with repeats
QSETS = (Q1, Q5, Q16)


def bits(t):
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def vp(t):
    return C.c_void_p(t.data_ptr())


def qarr(q):
    return (C.c_double * len(q))(*q)


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


def n_columns(n, group):
    return -(-n // min(group, n)) if n else 0


def stage(eng, rows, group, q):
    """sgx_quantile_mags over float32 rows [frames][pairs][M][2] on the device -> [columns][n_q][pairs][M][2], *n_out and guards checked"""
    import torch

    eng.use_current_stream()
    n = rows.numel() // (eng.pairs * eng.M * 2)
    cols = n_columns(n, group)
    g = Guarded(eng, cols * len(q) * eng.pairs * eng.M * 2)
    got = C.c_size_t(7)
    eng._check(eng._lib.sgx_quantile_mags(eng._ctx, vp(rows), n, group, qarr(q), C.c_uint32(len(q)), vp(g.out), C.byref(got)))
    torch.cuda.current_stream().synchronize()
    assert got.value == cols
    assert g.guards_untouched(), "sgx_quantile_mags wrote outside its output"
    return g.out.view(cols, len(q), eng.pairs, eng.M, 2)


def batch(eng, pcm, group, q, first_frame=0, max_frames=None):
    """sgx_quantile_batch -> [columns][n_q][pairs][M][2], *n_out and the guards checked"""
    import torch

    eng.use_current_stream()
    n_samples = pcm.numel() // eng.channels
    n = max(eng.num_frames(n_samples) - first_frame, 0)
    if max_frames is not None:
        n = min(n, max_frames)
    cols = n_columns(n, group)
    g = Guarded(eng, cols * len(q) * eng.pairs * eng.M * 2)
    got = C.c_size_t(7)
    eng._check(eng._lib.sgx_quantile_batch(eng._ctx, vp(pcm), n_samples, first_frame, 2 ** 40 if max_frames is None else max_frames, group,
                                           qarr(q), C.c_uint32(len(q)), vp(g.out), C.byref(got)))
    torch.cuda.current_stream().synchronize()
    assert got.value == cols
    assert g.guards_untouched(), "sgx_quantile_batch wrote outside its output"
    return g.out.view(cols, len(q), eng.pairs, eng.M, 2)


# ---- 1: the stage call on crafted rows ----------------------------------------------------------------------------------------------------
KINDS = ("random", "constant", "ties_below", "ties_above", "ascending", "descending", "specials", "first_frame", "last_frame", "both_ends")


def crafted(n, elems, q, rng):
    """[n][elems] float32: flat element e holds a column of kind KINDS[e % 10], so one call meets every kind in every part of a tile"""
    t = np.arange(n, dtype=np.float32)[:, None]
    e = np.arange(elems)
    ranks = sorted({ref.rank(x, n) for x in q})
    rows = rng.random((n, elems), dtype=np.float32)
    kind = e % len(KINDS)
    rows[:, kind == 1] = 0.25
    # two values: `low` frames hold 1, the others 2, in a shuffled order; low = k and k + 1 put the tie count on either side of rank k
    order = rng.permuted(np.tile(np.arange(n)[:, None], (1, elems)), axis=0)
    low = np.array([ranks[(i // len(KINDS)) % len(ranks)] for i in e]) + (kind == 3)
    two = np.where(order < low[None, :], 1.0, 2.0).astype(np.float32)
    rows[:, (kind == 2) | (kind == 3)] = two[:, (kind == 2) | (kind == 3)]
    rows[:, kind == 4] = (t + e[None, kind == 4] % 7).astype(np.float32)
    rows[:, kind == 5] = (n - t + e[None, kind == 5] % 7).astype(np.float32)
    for c in e[kind == 6]:                                                        # one NaN, one +inf, +0 and -0 mixed in
        where = rng.permutation(n)[:4]
        for w, v in zip(where, (np.nan, np.inf, 0.0, -0.0)):
            rows[w, c] = v
    rows[:, kind >= 7] = 1.0                                                      # the one distinguishing value in the first / last frame
    rows[0, kind == 7] = 0.5
    rows[n - 1, kind == 8] = 2.0
    rows[0, kind == 9] = 2.0
    rows[n - 1, kind == 9] = 0.5
    return rows


STAGE_WINDOWS = {   # M: engine keyword arguments.  4 channels are two pairs (the pair stride); a row is pairs * M * 2 floats, always even
    3: dict(window_samples=4, hop_samples=1, channels=4),          # 12 floats: below one tile
    16: dict(window_samples=17, hop_samples=4, channels=4),        # 64 floats: exactly one tile
    33: dict(window_samples=34, hop_samples=8, channels=2),        # 66 floats: a tile plus one (l, r) element
    255: dict(window_samples=256, hop_samples=64, channels=4),
    256: dict(window_samples=257, hop_samples=64, channels=4),     # 1024 floats: sixteen whole tiles
    257: dict(window_samples=258, hop_samples=64, channels=4),
    2047: dict(window_samples=2048, hop_samples=256, channels=4),
}
COLUMN_LENGTHS = (1, 2, 3, 63, 64, 65, LDS_FRAMES - 1, LDS_FRAMES, LDS_FRAMES + 1, 3 * LDS_FRAMES + 7)


def check_stage(eng, rows, group, qsets, what):
    import torch

    dev = torch.from_numpy(rows).to(eng.device)
    for q, want in zip(qsets, ref.quantiles_of_sets(rows, group, qsets)):
        got = stage(eng, dev, group, q)
        if not np.array_equal(bits(got), np_bits(want)):
            g = got.cpu().numpy().reshape(want.shape[0], len(q), -1).view(np.uint32)
            w = want.reshape(want.shape[0], len(q), -1).view(np.uint32)
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}, n_q {len(q)}: {len(bad)} words differ from the reference; first (column, q, element, kind): "
                                 f"{[(int(c), int(i), int(x), KINDS[int(x) % len(KINDS)]) for c, i, x in bad[:6]]}")


@pytest.mark.parametrize("M", sorted(STAGE_WINDOWS))
def test_stage_on_crafted_rows(M):
    eng = SpectrogramEngine(SR, device=0, **STAGE_WINDOWS[M])
    assert eng.M == M
    elems = eng.pairs * M * 2
    assert {3: elems < TILE, 16: elems == TILE, 33: elems == TILE + 2, 256: elems % TILE == 0}.get(M, elems % TILE != 0)
    rng = np.random.default_rng(M)
    every_q = Q1 + Q5 + Q16                                                       # the ties are placed around the ranks of all three sets
    for n in COLUMN_LENGTHS:
        rows = crafted(n, elems, every_q, rng).reshape(n, eng.pairs, M, 2)
        check_stage(eng, rows, n, QSETS, f"M {M}, one column of {n} frames")
    # several columns and a short last one on either path; group = SIZE_MAX is one column
    for n, group in ((3 * 65 + 7, 65), (2 * (LDS_FRAMES + 1) + 5, LDS_FRAMES + 1), (70, SIZE_MAX), (LDS_FRAMES + 30, SIZE_MAX), (9, 1)):
        rows = crafted(n, elems, Q5, rng).reshape(n, eng.pairs, M, 2)
        check_stage(eng, rows, group, (Q5,), f"M {M}, {n} frames in columns of {group}")
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


def noise(eng, frames, seed):
    n = eng.W + (frames - 1) * eng.H
    return eng.white_noise(n, seed=seed).reshape(-1).contiguous()


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
    pcm = noise(eng, frames, seed=0x51A7 + len(label))
    rows = eng.stft_batch(pcm)
    torch.cuda.synchronize()
    host = rows.cpu().numpy()
    host.setflags(write=False)
    return eng, pcm, rows, host


FLAG_CONTEXTS = {   # SGX_FLAG_PAIRED_FRAMES, SGX_FLAG_COMPLEX_MONO (rows of tests/edge_signals.py) and SGX_FLAG_NO_FUSED_RENDER
    "paired_frames": lambda: es.ROUTE["k1_paired_mono"].engine_kwargs(),
    "complex_mono": lambda: es.ROUTE["k1_complex_mono"].engine_kwargs(),
    "no_fused_render": lambda: dict(es.ROUTE["k1_lr_h256"].engine_kwargs(), fused_render=False),
}


def check_batch(eng, pcm, rows, host, frames, label):
    import torch

    for group in (1, 5, 32, 33, frames, frames + 10):
        got = batch(eng, pcm, group, Q5)
        assert got.shape == (n_columns(frames, group), 5, eng.pairs, eng.M, 2)
        staged = stage(eng, rows, group, Q5)
        assert np.array_equal(bits(got), bits(staged)), f"{label}/group {group}: the batch call differs from the stage call over its own rows"
        assert np.array_equal(bits(got), np_bits(ref.quantiles(host, group, Q5))), f"{label}/group {group}: not the reference's bits"
        if group == 1:
            for i in range(5):
                assert np.array_equal(bits(got[:, i]), bits(rows)), f"{label}: group 1, q {Q5[i]} is not the row"
        g = min(group, frames)                                                     # q = 0 and q = 1 are torch's minimum and maximum:
        whole = frames // g                                                        # the whole columns, then the short last one
        for c0, cols in ((0, rows[:whole * g].view(whole, g, eng.pairs, eng.M, 2)), (whole, rows[whole * g:][None])):
            if cols.shape[1]:
                part = got[c0:c0 + cols.shape[0]]
                assert torch.equal(part[:, 0].view(torch.int32), torch.amin(cols, 1).view(torch.int32)), f"{label}/group {group}: q = 0"
                assert torch.equal(part[:, 4].view(torch.int32), torch.amax(cols, 1).view(torch.int32)), f"{label}/group {group}: q = 1"
    for q in (Q1, Q16):
        got = batch(eng, pcm, 33, q)
        assert np.array_equal(bits(got), np_bits(ref.quantiles(host, 33, q))), f"{label}/n_q {len(q)}: not the reference's bits"


@pytest.mark.parametrize("label", sorted(FAMILY_ROUTES))
def test_batch_on_every_family(label):
    eng, pcm, rows, host = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    check_batch(eng, pcm, rows, host, frames, label)
    if eng.channels == 1:                                                         # (no family of this table sets SGX_FLAG_PAIRED_FRAMES)
        got = batch(eng, pcm, 5, Q5).cpu().numpy().view(np.uint32)
        assert np.array_equal(got[..., 0], got[..., 1]), f"{label}: a mono stream does not hold (v, v)"


@pytest.mark.parametrize("name", sorted(FLAG_CONTEXTS))
def test_batch_under_the_flags(name):
    import torch

    kw = FLAG_CONTEXTS[name]()
    assert any(kw.get(k) is v for k, v in (("paired_frames", True), ("complex_mono", True), ("fused_render", False))), kw
    eng = SpectrogramEngine(SR, device=0, **kw)
    frames = 40
    pcm = noise(eng, frames, seed=0x77 + len(name))
    rows = eng.stft_batch(pcm)
    torch.cuda.synchronize()
    check_batch(eng, pcm, rows, rows.cpu().numpy(), frames, name)
    if name == "paired_frames":                                                   # each side holds what its rows hold, not (v, v)
        got = batch(eng, pcm, 5, Q5)
        assert np.array_equal(bits(got), np_bits(ref.quantiles(rows.cpu().numpy(), 5, Q5)))
    eng.close()


@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "generic", "w16384"])
def test_identical_frames_return_the_row(label):
    """a signal whose period divides the hop: every frame sees the same samples.  Wherever the column's words are bitwise identical (a
    kernel that pairs frames in one transform may round the two of a pair differently) every q returns that word"""
    import torch

    eng = family_context(label)[0]
    frames = 33
    n = eng.W + (frames - 1) * eng.H
    period = 4
    assert eng.H % period == 0
    t = torch.arange(n, device=eng.device)
    wave = torch.tensor([0.5, -0.2, 0.31, -0.4], dtype=torch.float32, device=eng.device)[t % period]
    pcm = wave[:, None].repeat(1, eng.channels).reshape(-1).contiguous()
    rows = eng.stft_batch(pcm).view(torch.int32)
    same = (rows == rows[0]).all(0)
    share = float(same.float().mean())
    print(f"{label}: {share:.3f} of the elements hold one word in all {frames} frames")
    assert share > 0.0
    got = batch(eng, pcm, frames, Q16).view(torch.int32)
    for i in range(16):
        assert torch.equal(got[0, i][same], rows[0][same]), f"{label}: q {Q16[i]}"
    assert np.array_equal(bits(got.view(torch.float32)), np_bits(ref.quantiles(rows.view(torch.float32).cpu().numpy(), frames, Q16)))


# ---- 3: splits and seams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "w4800", "w16384", "large"])
def test_calls_split_at_column_boundaries_equal_one_call(label):
    eng, pcm, _, _ = family_context(label)
    frames = FAMILY_ROUTES[label][2]
    for group in (5, 7):
        full = batch(eng, pcm, group, Q5)
        cut = (n_columns(frames, group) // 2) * group
        parts = [batch(eng, pcm, group, Q5, max_frames=cut), batch(eng, pcm, group, Q5, first_frame=cut)]
        assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(full)), f"{label}: group {group} split at frame {cut}"
        parts = [batch(eng, pcm, group, Q5, first_frame=group, max_frames=group), batch(eng, pcm, group, Q5, first_frame=2 * group)]
        assert np.array_equal(np.concatenate([bits(p) for p in parts]), bits(full[1:])), f"{label}: group {group} from column 1"


@functools.lru_cache(maxsize=None)
def ch8_context():
    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=16, channels=8)
    cap = ref.cap(eng.pairs * eng.M * 8)
    assert cap == 3073 and eng._lib.sgx_quantile_max_group(eng._ctx) == cap
    return eng, cap


def test_range_seam_at_w2048_ch8():
    """8 channels: a frame's rows are 65 504 bytes and 3073 fit the workspace.  At group 33 a range holds 93 columns (3069 frames); 3300
    frames are one full range and a short one of 231 frames (7 columns).  White noise: every frame differs, so a column placed one slot
    early cannot pass.  Compared on the device"""
    import torch

    eng, cap = ch8_context()
    frames, group = 3300, 33
    plan = ref.plan(frames, group, eng.pairs * eng.M * 8)
    assert [(f, m) for f, m, _ in plan] == [(0, 3069), (3069, 231)] and frames > cap
    pcm = noise(eng, frames, seed=31)
    rows = eng.stft_batch(pcm)
    q = (0.5, 0.1)
    got = batch(eng, pcm, group, q)
    staged = stage(eng, rows, group, q)
    assert torch.equal(got.view(torch.int32), staged.view(torch.int32)), "the batch call across the range seam differs from the stage call"
    for col in (92, 93, 99):                                                      # the reference on the columns either side of the seam, and the last
        want = ref.quantiles(rows[col * group:(col + 1) * group].cpu().numpy(), group, q)
        assert np.array_equal(bits(got[col]), np_bits(want)), f"column {col}"
    # a short last column behind the seam, and a call split on the seam
    short = batch(eng, pcm, group, q, max_frames=3069 + 40)
    assert short.shape[0] == 95 and torch.equal(short[:94].view(torch.int32), got[:94].view(torch.int32))
    assert np.array_equal(bits(short[94]), np_bits(ref.quantiles(rows[3102:3109].cpu().numpy(), group, q)))
    parts = [batch(eng, pcm, group, q, max_frames=3069), batch(eng, pcm, group, q, first_frame=3069)]
    assert torch.equal(torch.cat(parts).view(torch.int32), got.view(torch.int32))
    torch.cuda.synchronize()


def test_the_group_cap():
    """group = cap is one column selected where its rows lie in the workspace (path B); group = cap + 1 on cap + 1 frames is refused"""
    import torch

    eng, cap = ch8_context()
    assert cap > LDS_FRAMES
    pcm = noise(eng, cap + 1, seed=32)
    n = pcm.numel() // eng.channels
    q = (0.0, 0.5, 1.0)
    got = batch(eng, pcm, cap, q, max_frames=cap)
    assert got.shape[0] == 1
    rows = eng.stft_batch(pcm)[:cap]
    ordered = torch.sort(rows, dim=0).values                                      # (rows of noise: finite and > 0, the numeric order is the key's)
    want = torch.stack([ordered[ref.rank(x, cap)] for x in q])
    assert torch.equal(got[0].view(torch.int32), want.view(torch.int32)), "one column of cap frames"
    del ordered, want
    # one frame more: refused, nothing written, the message names the cap
    words = 2 * len(q) * eng.pairs * eng.M * 2
    g = Guarded(eng, words)
    n_out = C.c_size_t(7)
    for group in (cap + 1, SIZE_MAX):
        rc = eng._lib.sgx_quantile_batch(eng._ctx, vp(pcm), n, 0, 2 ** 40, group, qarr(q), C.c_uint32(len(q)), vp(g.out), C.byref(n_out))
        assert rc == _lib.SGX_ERR_UNSUPPORTED and n_out.value == 0
        msg = eng._lib.sgx_last_error(eng._ctx)
        assert b"sgx_quantile_batch" in msg and str(cap).encode() in msg and b"sgx_quantile_max_group" in msg, msg
    torch.cuda.synchronize()
    assert g.untouched(), "a refused call wrote to its buffer"
    # ... while cap + 1 frames in columns of cap are two columns, and the same context serves it
    again = batch(eng, pcm, cap, q)
    assert again.shape[0] == 2 and torch.equal(again[0].view(torch.int32), got[0].view(torch.int32))
    last = eng.stft_batch(pcm)[cap]
    for i in range(len(q)):
        assert torch.equal(again[1, i].view(torch.int32), last.view(torch.int32))
    # the stage call takes the longer column
    staged = stage(eng, eng.stft_batch(pcm), SIZE_MAX, (1.0,))
    assert torch.equal(staged[0, 0].view(torch.int32), torch.amax(eng.stft_batch(pcm), 0).view(torch.int32))


@pytest.mark.parametrize("kw", [dict(window_samples=2048, hop_samples=256, channels=1), dict(window_samples=2048, hop_samples=256, channels=2),
                                dict(window_samples=2400, hop_samples=93, channels=4), dict(window_samples=64, hop_samples=16, channels=2)],
                         ids=lambda kw: f"w{kw['window_samples']}_ch{kw['channels']}")
def test_max_group_is_the_workspace_in_rows(kw):
    eng = SpectrogramEngine(SR, device=0, **kw)
    cap = eng._lib.sgx_quantile_max_group(eng._ctx)
    assert cap == (192 << 20) // (eng.pairs * eng.M * 2 * 4) == eng.quantile_max_group
    if kw["window_samples"] == 2048:
        assert cap == 12294
    eng.close()
    assert _lib.load().sgx_quantile_max_group(None) == 0


def test_a_row_longer_than_the_workspace():
    """W 2048 with 32 768 channels: one frame's rows are 268 MB, more than the workspace.  The cap is 1 and a group-1 call is the rows"""
    import torch

    eng = SpectrogramEngine(SR, device=0, window_samples=2048, hop_samples=256, channels=32768)
    assert eng.pairs * eng.M * 8 > 192 << 20 and eng._lib.sgx_quantile_max_group(eng._ctx) == 1
    pcm = noise(eng, 2, seed=33)
    got = batch(eng, pcm, 1, Q1)
    assert got.shape[0] == 2
    rows = eng.stft_batch(pcm)
    assert torch.equal(got[:, 0].view(torch.int32), rows.view(torch.int32))
    n_out = C.c_size_t(7)
    g = Guarded(eng, 16)
    rc = eng._lib.sgx_quantile_batch(eng._ctx, vp(pcm), pcm.numel() // eng.channels, 0, 2, 2, qarr(Q1), C.c_uint32(1), vp(g.out), C.byref(n_out))
    assert rc == _lib.SGX_ERR_UNSUPPORTED and n_out.value == 0 and g.untouched()
    del got, rows, pcm
    eng.close()
    torch.cuda.empty_cache()


# ---- 4: independence of compute-unit limit, run claim and stream ---------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["wg4096_real_h256", "wg4096_lr", "wg4096_ch4", "w4800", "w16384"])
def test_cu_limits(label):
    import torch

    eng, pcm, _, host = family_context(label)
    try:
        for group in (5, 33):
            expect = np_bits(ref.quantiles(host, group, Q5))
            for limit in (1, 3, 255, 0):
                eng.set_cu_limit(limit)
                assert np.array_equal(bits(batch(eng, pcm, group, Q5)), expect), f"{label}/group {group}: {limit} compute units"
    finally:
        eng.set_cu_limit(0)
    torch.cuda.synchronize()


def test_run_claims_on_the_mono_w2048_context():
    eng, pcm, _, host = family_context("wg4096_real_h256")
    expect = np_bits(ref.quantiles(host, 33, Q5))
    try:
        eng.set_run_claim(16, 0)
        static = bits(batch(eng, pcm, 33, Q5))
        eng.set_run_claim(4, 8)
        claimed = bits(batch(eng, pcm, 33, Q5))
    finally:
        eng.set_run_claim(0, 0)
    assert np.array_equal(static, expect) and np.array_equal(claimed, expect)


@pytest.mark.parametrize("label", ["wg4096_lr", "w16384"])
def test_on_a_stream_held_back_by_pending_work(label):
    """queued behind a long kernel on a non-default stream, both calls return before that kernel ends; the PCM is written on the same
    stream behind the sleep and is NaN until then, so a kernel put on any other stream would select among NaNs"""
    import torch

    name, _, frames = FAMILY_ROUTES[label]
    eng = SpectrogramEngine(SR, device=0, **es.ROUTE[name].engine_kwargs())
    n = eng.W + (frames - 1) * eng.H
    clean = eng.white_noise(n, seed=21)
    want_batch = batch(eng, clean.reshape(-1), 33, Q5)                            # (the workspace is grown here)
    rows_ref = eng.stft_batch(clean.reshape(-1))
    torch.cuda.synchronize()
    pcm = torch.full((n * eng.channels,), float("nan"), dtype=torch.float32, device=eng.device)
    rows = torch.full_like(rows_ref, float("nan"))
    outs = [Guarded(eng, want_batch.numel()), Guarded(eng, want_batch.numel())]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    eng.set_stream(s.cuda_stream)
    lib, got = eng._lib, C.c_size_t(0)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(400_000_000)
        eng._check(lib.sgx_synth_white_noise(eng._ctx, vp(pcm), 0, n, eng.channels, 21))
        eng._check(lib.sgx_quantile_batch(eng._ctx, vp(pcm), n, 0, frames, 33, qarr(Q5), C.c_uint32(5), vp(outs[0].out), C.byref(got)))
        eng._check(lib.sgx_stft_batch(eng._ctx, vp(pcm), n, 0, frames, vp(rows), None))
        eng._check(lib.sgx_quantile_mags(eng._ctx, vp(rows), frames, 33, qarr(Q5), C.c_uint32(5), vp(outs[1].out), None))
        done = torch.cuda.Event()
        done.record(s)
        assert not done.query(), f"{label}: a call waited for the stream"
        eng.sync()
        assert got.value == n_columns(frames, 33)
        for g, who in zip(outs, ("batch", "stage")):
            assert g.guards_untouched() and np.array_equal(bits(g.out), bits(want_batch)), f"{label}: {who}"
    finally:
        eng.set_stream(0)
        eng.close()


# ---- 5: truth -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_the_median_ignores_a_click_and_the_mean_does_not(channels):
    """W 256, hop 32: a sinusoid at the centre of bin 64 of the 512-point transform (period 8 divides the hop, so every clean frame sees the
    same samples) and one full-scale click.  The click touches W / H = 8 consecutive frames of the 33-frame column, fewer than the 16 that
    could move rank 16.  (The premise was checked on the CPU with the oracle: 8 frames touched, the median between the clean frames' own
    extremes, the mean of the powers off by far more than the tolerance.)"""
    import torch

    W, H, frames, k = 256, 32, 33, 64
    eng = SpectrogramEngine(SR, device=0, window_samples=W, hop_samples=H, channels=channels)
    n = W + (frames - 1) * H
    t = np.arange(n)
    tone = (0.25 * np.cos(2.0 * np.pi * k * t / (2 * W))).astype(np.float32)
    clicked = tone.copy()
    at = n // 2 + 5
    clicked[at] = 1.0
    touched = [f for f in range(frames) if f * H <= at < f * H + W]
    assert len(touched) == W // H == 8 and len(touched) < ref.rank(0.5, frames) == 16
    clean = [f for f in range(frames) if f not in touched]
    pcm = torch.from_numpy(np.repeat(clicked[:, None], channels, 1).reshape(-1).copy()).to(eng.device)
    rows = eng.stft_batch(pcm).cpu().numpy()
    median = batch(eng, pcm, frames, Q1).cpu().numpy()[0, 0]
    # exact: the median is one of the untouched frames' own words, or lies between two of them
    lo, hi = rows[clean].min(0), rows[clean].max(0)
    assert ((median >= lo) & (median <= hi)).all(), "the median left the range of the untouched frames"
    truth = oracle.np_truth_frame(np.stack([tone[:W]] * 2, 1), W)                 # float64, [M][2]
    worst = mags_error(median[0], truth, FLOOR_WIDE)
    print(f"ch {channels}: worst |median - truth| / allowance = {worst:.3f}")
    assert worst <= 1.0
    # the Welch mean of the same column is not the clean power: the allowance of REL_TOL carried to the square
    psd = eng.psd_batch(pcm, frames).cpu().numpy().astype(np.float64)[0, 0]
    e = REL_TOL * np.maximum(np.abs(truth), FLOOR_WIDE * np.abs(truth).max())
    allow = 2.0 * np.abs(truth) * e + e * e
    off = np.abs(psd - truth * truth) / allow
    print(f"ch {channels}: the mean's worst |psd - truth^2| / allowance = {off.max():.3g}; bins beyond it: {(off > 1.0).sum()}")
    assert (off > 1.0).any(), "the case does not discriminate: the mean holds the clean power too"
    eng.close()


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch

    eng, pcm, rows, host = family_context("wg4096_lr")
    frames = FAMILY_ROUTES["wg4096_lr"][2]
    n = pcm.numel() // eng.channels
    lib, bad = eng._lib, _lib.SGX_ERR_INVALID_ARG
    g = Guarded(eng, frames * 16 * eng.pairs * eng.M * 2)
    out = vp(g.out)
    got = C.c_size_t(7)

    def batch_call(ctx=eng._ctx, d_in=vp(pcm), group=5, q=Q5, n_q=None, d_out=out):
        return lib.sgx_quantile_batch(ctx, d_in, n, 0, 1000, group, qarr(q) if q is not None else None,
                                      C.c_uint32(len(q) if n_q is None else n_q), d_out, C.byref(got))

    def stage_call(ctx=eng._ctx, d_in=vp(rows), group=5, q=Q5, n_q=None, d_out=out):
        return lib.sgx_quantile_mags(ctx, d_in, frames, group, qarr(q) if q is not None else None,
                                     C.c_uint32(len(q) if n_q is None else n_q), d_out, C.byref(got))

    for call, who in ((batch_call, b"sgx_quantile_batch"), (stage_call, b"sgx_quantile_mags")):
        for kw in (dict(group=0), dict(n_q=0), dict(q=(0.5,) * 17), dict(q=(0.5, -0.1)), dict(q=(1.0000001,)), dict(q=(0.1, float("nan"))),
                   dict(q=None, n_q=3), dict(d_out=None), dict(d_in=None)):
            got.value = 7
            assert call(**kw) == bad, (who, kw)
            assert who in lib.sgx_last_error(eng._ctx), (who, kw, lib.sgx_last_error(eng._ctx))
            assert got.value == 0, (who, kw)
        assert call(ctx=None) == bad
    # not errors: too few samples, no frame in range, no frames, a null n_out
    got.value = 7
    assert lib.sgx_quantile_batch(eng._ctx, vp(pcm), eng.W - 1, 0, 10, 5, qarr(Q5), C.c_uint32(5), out, C.byref(got)) == 0 and got.value == 0
    got.value = 7
    assert lib.sgx_quantile_batch(eng._ctx, vp(pcm), n, frames, 10, 5, qarr(Q5), C.c_uint32(5), out, C.byref(got)) == 0 and got.value == 0
    got.value = 7
    assert lib.sgx_quantile_mags(eng._ctx, vp(rows), 0, 5, qarr(Q5), C.c_uint32(5), out, C.byref(got)) == 0 and got.value == 0
    torch.cuda.synchronize()
    assert g.untouched(), "a refused or empty call wrote to its buffer"
    want = np_bits(ref.quantiles(host, 5, Q5))
    assert lib.sgx_quantile_batch(eng._ctx, vp(pcm), n, 0, 1000, 5, qarr(Q5), C.c_uint32(5), out, None) == 0
    torch.cuda.synchronize()
    assert g.guards_untouched() and np.array_equal(bits(g.out[:want.size]), want)
    assert lib.sgx_quantile_mags(eng._ctx, vp(rows), frames, 5, qarr(Q5), C.c_uint32(5), C.c_void_p(g.out.data_ptr() + 4), None) == 0
    torch.cuda.synchronize()                                                      # (no alignment beyond float's)
    assert g.guards_untouched() and np.array_equal(bits(g.out[1:1 + want.size]), want)


def test_python_methods():
    eng, pcm, rows, host = family_context("wg4096_ch4")
    got = eng.quantile_batch(pcm, 5, Q5, first_frame=5, max_frames=12)
    assert got.shape == (3, 5, eng.pairs, eng.M, 2)
    assert np.array_equal(bits(got), np_bits(ref.quantiles(host[5:17], 5, Q5)))
    assert np.array_equal(bits(eng.quantile_mags(rows[5:17].contiguous(), 5, Q5)), bits(got))
    assert np.array_equal(bits(eng.quantile_batch(pcm, 2 ** 64 - 1, 0.5)), np_bits(ref.quantiles(host, 40, (0.5,))))
    assert eng.quantile_max_group == (192 << 20) // (eng.pairs * eng.M * 8)
