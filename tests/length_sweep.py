"""Every transform length the library accepts, as data (a plain helper of tests/test_length_sweep.py and tests/test_gpu_lengths.py).

The transform length selects a plan that is built at run time: the stage list, the (RA, RB) radix pairs, the twiddle tables, the LDS
padding and the split table of the mixed-radix kernels (csrc/stft_mixed.hip: make_plan / build_tables), the convolution length of the
chirp-z kernels, the N1 x N2 factorisation and the sub-transform radices of kernel 11 (csrc/large_plan.hpp).  The sets below are derived
from those rules as the tests restate them -- nothing here asks the library:

  SMOOTH        every W in [4, 10240] with a 2-3-5-7-smooth 2W that a mixed-radix kernel serves by default, and W 2400 once more under
                mixed_generic
  POW2          W = 4 .. 8192 on the default route (where SMOOTH does not hold it already), under force_generic, and under
                complex_mono / paired_frames where those change the kernel
  CHIRP         per convolution class L = 16 .. 16384 (and per class of the mono real-input convolution) the class ends, every exact
                fit 3W - 1 = L, and four seeded lengths; the class ends again on the radix-4 ladder (force_generic)
  LARGE_DIRECT  a cover of kernel 11's direct plans: every distinct N1 and every distinct N2
  LARGE_CHIRP   per class L = 2^15 .. 2^22 of kernel 11's chirp-z the class ends and the exact fits

A Length names a window, the engine flags, the channel counts it runs with, and the route the GPU test asserts first: stft_kernel and the
render_path bits 2 (compile-time plan / chirp-z through the composite stages) and 3 (real-input mode, mono contexts only)."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass

import numpy as np

import edge_signals as es
from conftest import FLOOR_K16, FLOOR_WIDE, PEAK_FLOOR

MIX_MAX_P = 20480            # mixed_supported: 2W <= 20480 (the transform lives in LDS)
MIX_MAX_RADIX = 28           # kMaxRadix
MIX_LDS_BYTES = 160 * 1024
POW2_MIXED_MIN = 512         # kPow2MixedMin (sgx_api.hip): powers of two from here on ride the composite stages (but 2048: K1, 8192: K16)
CHIRP_MAX_L = 16384          # bluestein_supported / chirpz_supported: 3W - 1 <= 16384
CHIRP_STAGES_MIN_L = 512     # chirpz_supported: L = 512 .. 16384 run the composite stages, shorter ones the radix-4 ladder (W < 86)
LARGE_MAX_W = 1 << 20        # large_plan.hpp: kMaxW


def smooth7(n: int) -> bool:
    return es._smooth7(n)


# ---- the mixed-radix plan (moved here from tests/test_host_logic.py, which imports it back) -----------------------------------------
def mixed_radix_plan(P):
    """csrc/stft_mixed.hip make_plan restated: P's factors 7, 5, 4 (pairs of twos), 3 and a last 2, grouped into stages of
    one or two factors with a product <= 28 -- fewest stages, then the smallest largest radix, then the smallest sum."""
    n, factors = P, []
    for f in (7, 5):
        while n % f == 0:
            factors.append(f)
            n //= f
    threes = []
    while n % 3 == 0:
        threes.append(3)
        n //= 3
    while n % 4 == 0:
        factors.append(4)
        n //= 4
    factors += threes
    if n % 2 == 0:
        factors.append(2)
        n //= 2
    if n != 1:
        return None
    factors.sort(reverse=True)
    best = [None, None]

    def search(rest, cur):
        if not rest:
            prods = [a * b for a, b in cur]
            key = (len(cur), max(prods), sum(prods))
            if best[0] is None or key < best[0]:
                best[0], best[1] = key, list(cur)
            return
        f, rest = rest[-1], rest[:-1]
        search(rest, cur + [(f, 1)])
        for i, g in enumerate(rest):
            if (i > 0 and rest[i] == rest[i - 1]) or f * g > 28:
                continue
            search(rest[:i] + rest[i + 1:], cur + [(max(f, g), min(f, g))])

    search(factors, [])
    odd = lambda g: (g[0] * g[1]) & (g[0] * g[1] - 1) != 0  # noqa: E731
    return sorted(best[1], key=lambda g: (not odd(g), -(g[0] * g[1]) if odd(g) else g[0] * g[1]))


def mixed_pad_every(P: int, plan) -> int:
    """build_tables' padding rule restated: one point of padding per R_last points when R_last is even, the padded image fits the
    160 KB of LDS, and the padding costs no resident workgroup (counted up to four); else 0"""
    r_last = plan[-1][0] * plan[-1][1]

    def resident(points):
        return max(1, min(8, MIX_LDS_BYTES // (points * 8)))

    padded = P + P // r_last
    if r_last % 2 == 0 and padded * 8 <= MIX_LDS_BYTES and resident(padded) >= min(resident(P), 4):
        return r_last
    return 0


# MIX_FIXED_PLANS / MIX_FIXED4_PLANS of csrc/stft_mixed_kernels.hpp: P -> the compile-time stages (tests/test_length_sweep.py holds this table to
# the macros' text).  render_path bit 2 is set when the run-time rule arrives at exactly this plan, with R_last's padding.
MIX_FIXED = {
    4800: ((5, 4), (5, 3), (4, 4)), 4410: ((7, 3), (5, 3), (7, 2)), 3200: ((5, 4), (5, 2), (4, 4)), 1600: ((5, 4), (5, 1), (4, 4)),
    800: ((5, 2), (5, 1), (4, 4)), 8820: ((7, 3), (7, 3), (5, 4)), 2048: ((4, 2), (4, 4), (4, 4)), 1024: ((4, 1), (4, 4), (4, 4)),
    2400: ((5, 3), (5, 2), (4, 4)), 2205: ((7, 3), (5, 3), (7, 1)), 4096: ((4, 4), (4, 4), (4, 4)), 512: ((4, 1), (4, 2), (4, 4)),
    9600: ((4, 3), (5, 2), (5, 1), (4, 4)), 19200: ((5, 3), (5, 1), (4, 4), (4, 4)), 17640: ((5, 3), (7, 2), (4, 3), (7, 1)),
    8192: ((4, 1), (4, 2), (4, 4), (4, 4)),
}


def macro(name):
    """the X(...) argument lists of a #define in csrc/stft_mixed_kernels.hpp, continuation lines included (the tests hold the tables here to them)"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spectrogram_rs_amd", "csrc", "stft_mixed_kernels.hpp")
    m = re.search(r"#define " + name + r"\(X\)((?:.*\\\n)*.*)\n", open(src).read())
    assert m, name
    return [tuple(int(v) for v in args.split(",")) for args in re.findall(r"X\(([^)]*)\)", m.group(1))]


def mixed_is_fixed(P: int) -> bool:
    """is_plan of build_tables: the host's plan of P points is the compiled one, and pad_every is R_last (even) or 0 (odd)"""
    plan = mixed_radix_plan(P)
    if P not in MIX_FIXED or plan is None or tuple(plan) != MIX_FIXED[P]:
        return False
    r_last = plan[-1][0] * plan[-1][1]
    return mixed_pad_every(P, plan) == (r_last if r_last % 2 == 0 else 0)


# ---- one length of a set ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Length:
    W: int
    flags: tuple = ()          # SpectrogramEngine keyword flags set to True
    channels: tuple = (2, 1)   # one context per entry
    kernel: int = 0            # expected info.stft_kernel
    bit2: bool = False         # render_path bit 2 (value 4) set, on every channel count
    bit3_mono: bool = False    # render_path bit 3 (value 8) set on the mono context (never on two channels)
    floor: float = FLOOR_WIDE  # the conftest floor this kernel class is held to
    plan: tuple = ()           # mixed radix: the 2W-point plan; kernel 11: (L, N1, N2, chirp)
    plan_mono: tuple = ()      # mixed radix: the W-point plan of real-input mode
    L: int = 0                 # chirp-z: the convolution length of the (l, r) frame
    L_mono: int = 0            # chirp-z: the convolution length of real-input mode (0: the radix-4 ladder has none)
    ladder: bool = False       # chirp-z on the radix-4 ladder (W < 86, or force_generic)
    why: str = ""

    @property
    def key(self):
        return (self.W, self.flags)

    @property
    def H(self) -> int:
        return self.W // 3 + 1

    def engine_kwargs(self, channels: int) -> dict:
        kw = dict(window_samples=self.W, hop_samples=self.H, channels=channels, rows=16)
        kw.update({f: True for f in self.flags})
        return kw

    def bits(self, channels: int):
        """(bits that must be set, bits that must be clear) of render_path, among bits 2 and 3"""
        on = (es.R4 if self.bit2 else 0) | (es.R8 if self.bit3_mono and channels == 1 else 0)
        return on, (es.R4 | es.R8) & ~on


# ---- SMOOTH ------------------------------------------------------------------------------------------------------------------------------
def is_pow2(n: int) -> bool:
    return n & (n - 1) == 0


ALL_SMOOTH_W = [W for W in range(4, MIX_MAX_P // 2 + 1) if smooth7(2 * W)]
# the windows another kernel runs by default: the generic power-of-two kernel below kPow2MixedMin, K1 at 2048, K16 at 8192
SMOOTH_EXCLUDED = [W for W in ALL_SMOOTH_W if is_pow2(W) and (W < POW2_MIXED_MIN or W in (2048, 8192))]


def _smooth(W: int, flags=()) -> Length:
    plan = tuple(mixed_radix_plan(2 * W))
    half = mixed_radix_plan(W) if W >= 8 else None     # mixed_init: the W-point plan of real-input mode from W 8 on
    return Length(W, tuple(flags), kernel=9 if W == 2400 and not flags else 6, bit2=mixed_is_fixed(2 * W), bit3_mono=half is not None,
                  plan=plan, plan_mono=tuple(half) if half else ())


SMOOTH = [_smooth(W) for W in ALL_SMOOTH_W if W not in SMOOTH_EXCLUDED] + [_smooth(2400, ("mixed_generic",))]


# ---- POW2 --------------------------------------------------------------------------------------------------------------------------------
def _pow2() -> list:
    out = []
    for lg in range(2, 14):
        W = 1 << lg
        floor = PEAK_FLOOR if W == 2048 else FLOOR_WIDE    # (tests/edge_signals.py: K1 and the generic kernel at W 2048)
        if W in SMOOTH_EXCLUDED:   # the default route, where SMOOTH does not run it
            if W == 2048:
                out.append(Length(W, kernel=2, bit3_mono=True, floor=PEAK_FLOOR, why="K1 / K1R"))
            elif W == 8192:
                out.append(Length(W, kernel=10, floor=FLOOR_K16, why="K16"))
            else:
                out.append(Length(W, kernel=0, why="generic"))
        out.append(Length(W, ("force_generic",), kernel=0, floor=floor, why="generic (forced)"))
    # mono contexts whose flag changes the kernel: K1R -> K1 on (s, s) / on frame pairs, K16 on frame pairs, real-input mode -> the 2W plan
    out.append(Length(2048, ("complex_mono",), (1,), kernel=2, floor=PEAK_FLOOR, why="K1 on (s, s)"))
    out.append(Length(2048, ("paired_frames",), (1,), kernel=2, floor=PEAK_FLOOR, why="K1 on frame pairs"))
    out.append(Length(8192, ("paired_frames",), (1,), kernel=10, floor=FLOOR_K16, why="K16 on frame pairs"))
    for W in (512, 1024, 4096):
        out.append(Length(W, ("complex_mono",), (1,), kernel=6, bit2=mixed_is_fixed(2 * W), plan=tuple(mixed_radix_plan(2 * W)),
                          why="mixed radix on (s, s)"))
    return out


POW2 = _pow2()


# ---- CHIRP -------------------------------------------------------------------------------------------------------------------------------
def chirp_length(W: int) -> int:
    """chirp_length / bluestein_init: L = pow2 >= 3W - 1 (2W outputs of W non-zero inputs)"""
    L = 1
    while L < 3 * W - 1:
        L <<= 1
    return L


def chirp_length_mono(W: int) -> int:
    """ChirpTables::half (chirpz_init, conv_length): real-input mode is the chirp-z transform of W points over nz = ceil(W / 2) sample
    pairs: L = the power of two >= W + nz - 1, at least 512.  Its classes end at W 342, 683, 1366, 2731 (683 and 2731 fit exactly)"""
    L = 512
    while L < W + (W + 1) // 2 - 1:
        L <<= 1
    return L


def chirp_served(W: int) -> bool:
    """kernel 4 by default: 2W has a prime factor above 7 and 3W - 1 <= 16384"""
    return W >= 4 and not smooth7(2 * W) and 3 * W - 1 <= CHIRP_MAX_L


def _nearest(W: int, ok, lo: int, hi: int, prefer: int):
    """the nearest w in [lo, hi] with ok(w); ties go towards `prefer` (-1 / +1).  None if there is none"""
    for d in range(0, hi - lo + 1):
        for w in ((W + prefer * d, W - prefer * d) if d else (W,)):
            if lo <= w <= hi and ok(w):
                return w
    return None


def _class_members(lo: int, hi: int, seed, ok, last_class: bool) -> dict:
    """{W: why} of one class whose windows are lo .. hi: its last W, the first W past it, four seeded W (two odd, two even) -- each moved
    to the nearest W that ok() accepts, the class ends without leaving their class"""
    out = {}
    w = _nearest(hi, ok, lo, hi, -1)
    if w is not None:
        out[w] = "largest W of the class"
    if not last_class:
        w = _nearest(hi + 1, ok, hi + 1, 2 * hi + 1, +1)
        if w is not None:
            out.setdefault(w, "first W of the next class")
    rng = np.random.default_rng(seed)
    for parity in (1, 1, 0, 0):
        if hi - lo < 4:
            break
        for _ in range(64):
            w = int(rng.integers(lo, hi + 1))
            w = _nearest(w, lambda v: ok(v) and v % 2 == parity, lo, hi, +1)
            if w is not None and w not in out:
                out[w] = "seeded"
                break
    return out


CHIRP_SEED = 20240
CHIRP_EXACT = [11, 43, 171, 683, 2731]              # 3W - 1 = 32, 128, 512, 2048, 8192
CHIRP_MONO_EXACT = [683, 2731]                      # W + ceil(W / 2) - 1 = 1024, 4096
CHIRP_CLASSES = [1 << k for k in range(4, 15)]      # L = 16 .. 16384
CHIRP_MONO_CLASSES = [512, 1024, 2048, 4096, 8192]


def _chirp() -> list:
    why = {}
    ends = set()
    for L in CHIRP_CLASSES:                          # W of class L: L / 2 < 3W - 1 <= L
        lo, hi = max((L // 2 + 1) // 3 + 1, 4), (L + 1) // 3
        m = _class_members(lo, hi, [CHIRP_SEED, L], chirp_served, last_class=L == CHIRP_MAX_L)
        ends.update(w for w, y in m.items() if y != "seeded")
        for w, y in m.items():
            why.setdefault(w, f"L {L}: {y}")
    for L in CHIRP_MONO_CLASSES:                     # W of mono class L: L / 2 < W + ceil(W / 2) - 1 <= L (the first class starts at W 86)
        hi = max(w for w in range(4, (CHIRP_MAX_L + 1) // 3 + 1) if chirp_length_mono(w) <= L)
        lo = 86 if L == 512 else 1 + max(w for w in range(4, hi) if chirp_length_mono(w) < L)
        m = _class_members(lo, hi, [CHIRP_SEED, 1, L], chirp_served, last_class=L == 8192)
        for w, y in m.items():
            why.setdefault(w, f"mono L {L}: {y}")
    for w in sorted(set(CHIRP_EXACT + CHIRP_MONO_EXACT)):
        assert chirp_served(w)
        why[w] = why.get(w, "") + " (exact fit)"
        ends.add(w)
    out = []
    for W in sorted(why):
        stages = chirp_length(W) >= CHIRP_STAGES_MIN_L
        out.append(Length(W, kernel=4, bit2=stages, bit3_mono=stages, L=chirp_length(W), L_mono=chirp_length_mono(W) if stages else 0,
                          ladder=not stages, why=why[W].strip()))
    for W in sorted(ends):                            # the class ends of the composite stages again on the radix-4 ladder
        if chirp_length(W) >= CHIRP_STAGES_MIN_L:
            out.append(Length(W, ("force_generic",), kernel=4, L=chirp_length(W), ladder=True, why="the ladder at a class end"))
    return out


CHIRP = _chirp()


# ---- kernel 11 ---------------------------------------------------------------------------------------------------------------------------
LARGE_DIRECT_ALL = [P // 2 for P in range(MIX_MAX_P + 2, 2 * LARGE_MAX_W + 1, 2) if smooth7(P)]   # the 944 direct plans


def _large_direct() -> list:
    out, seen1, seen2 = [], set(), set()
    for W in LARGE_DIRECT_ALL:                        # ascending: keep a length whose N1 is new as an N1 or whose N2 is new as an N2
        L, N1, N2, chirp = es.large_plan(W)
        assert not chirp
        if N1 not in seen1 or N2 not in seen2:
            seen1.add(N1)
            seen2.add(N2)
            out.append(Length(W, ("large_transforms",), (2,), kernel=11, plan=(L, N1, N2, False)))
    return out


LARGE_DIRECT = _large_direct()
LARGE_CHIRP_EXACT = [10923, 43691, 174763, 699051]  # 3W - 1 = 2^15, 2^17, 2^19, 2^21
LARGE_CHIRP_CLASSES = [1 << k for k in range(15, 23)]


def large_chirp_served(W: int) -> bool:
    """kernel 11's chirp-z: no in-LDS kernel serves W (3W - 1 > 16384) and 2W has a prime factor above 7"""
    return 3 * W - 1 > CHIRP_MAX_L and W <= LARGE_MAX_W and not smooth7(2 * W)


def _large_chirp() -> list:
    why = {}
    for L in LARGE_CHIRP_CLASSES:
        lo, hi = (L // 2 + 1) // 3 + 1, min((L + 1) // 3, LARGE_MAX_W)
        w = _nearest(hi, large_chirp_served, lo, hi, -1)
        why.setdefault(w, f"L {L}: largest W of the class")
        w = _nearest(lo, large_chirp_served, lo, hi, +1)
        why.setdefault(w, f"L {L}: first W of the class")
    for w in LARGE_CHIRP_EXACT:
        assert large_chirp_served(w) and 3 * w - 1 == chirp_length(w)
        why[w] = why.get(w, f"L {chirp_length(w)}:") + " (exact fit)"
    return [Length(W, ("large_transforms",), (2,), kernel=11, plan=es.large_plan(W), L=chirp_length(W), why=why[W]) for W in sorted(why)]


LARGE_CHIRP = _large_chirp()

SETS = {"SMOOTH": SMOOTH, "POW2": POW2, "CHIRP": CHIRP, "LARGE_DIRECT": LARGE_DIRECT, "LARGE_CHIRP": LARGE_CHIRP}


# ---- chunks: what one case of the GPU sweep runs -------------------------------------------------------------------------------------------
def _runs(entries, n):
    return [entries[i:i + n] for i in range(0, len(entries), n)]


def chunks() -> dict:
    """{case id: [Length, ...]}: SMOOTH in ranges of 2W, POW2 by route, CHIRP by class, LARGE_DIRECT in runs of 16 with the eight longest
    on their own, LARGE_CHIRP by class"""
    out = {}
    for run in _runs(SMOOTH[:-1], 22):
        out[f"smooth-2W-{2 * run[0].W}-{2 * run[-1].W}"] = run
    out["smooth-2W-4800-mixed_generic"] = [SMOOTH[-1]]
    out["pow2-default"] = [e for e in POW2 if not e.flags]
    out["pow2-force_generic"] = [e for e in POW2 if e.flags == ("force_generic",)]
    out["pow2-mono-modes"] = [e for e in POW2 if e.flags and e.flags != ("force_generic",)]
    for L in CHIRP_CLASSES:
        run = [e for e in CHIRP if e.L == L]
        if run:
            out[f"chirp-L-{L}"] = run
    direct = sorted(LARGE_DIRECT, key=lambda e: e.W)
    for run in _runs(direct[:-8], 16):
        out[f"large-direct-W-{run[0].W}-{run[-1].W}"] = run
    for e in direct[-8:]:
        out[f"large-direct-W-{e.W}"] = [e]
    for L in LARGE_CHIRP_CLASSES:
        out[f"large-chirp-L-{L}"] = [e for e in LARGE_CHIRP if e.L == L]
    return out


# ---- the stream and the samples the round trip is held on ------------------------------------------------------------------------------------
def stream(e: Length, channels: int, frames: int, seed=None) -> np.ndarray:
    """[n][channels] float32: `frames` frames at hop W // 3 + 1 and a ragged tail of H - 1 samples, white noise of seed W at half scale"""
    import oracle
    n = (frames - 1) * e.H + e.W + e.H - 1
    return (oracle.white_noise(n * channels, seed=e.W if seed is None else seed) * np.float32(0.5)).reshape(n, channels)


def local_peak_at(x: np.ndarray, W: int, lo: int, hi: int) -> np.ndarray:
    """test_gpu_istft.local_peak(x, W)[lo:hi] -- max |x| over [n - W, n + W] and the channel pair -- in linear time: the zero-padded stream
    is cut into blocks of 2W + 1 samples, and a window's maximum is that of a block's tail and the next block's head"""
    m = np.abs(np.asarray(x, np.float64))
    if m.shape[1] >= 2:
        m = np.repeat(m.reshape(m.shape[0], -1, 2).max(axis=2), 2, axis=1)
    B = 2 * W + 1
    n_blocks = -(-(m.shape[0] + 2 * W) // B)
    pad = np.zeros((n_blocks * B, m.shape[1]))
    pad[W:W + m.shape[0]] = m
    blocks = pad.reshape(n_blocks, B, -1)
    head = np.maximum.accumulate(blocks, axis=1).reshape(pad.shape)
    tail = np.maximum.accumulate(blocks[:, ::-1], axis=1)[:, ::-1].reshape(pad.shape)
    n = np.arange(lo, hi)                        # the window of sample n is pad[n : n + B]
    return np.maximum(tail[n], head[n + B - 1])


def independent_float32_ratio(lr: np.ndarray, W: int, floor: float) -> float:
    """mags_error of an independent float32 transform of the same windowed frame (numpy's pocketfft on complex64, which stays complex64)
    against the float64 truth: what any float32 FFT of this frame can be expected to read"""
    from conftest import mags_error
    win = es.hann(W)
    lr = np.ascontiguousarray(lr, np.float32).reshape(-1, 2)[:W]
    z = ((lr[:, 0] * win) + 1j * (lr[:, 1] * win)).astype(np.complex64)
    F = np.fft.fft(np.concatenate([z, np.zeros(W, np.complex64)]))
    assert F.dtype == np.complex64
    k = np.arange(1, W)
    a, b = F[k], F[2 * W - k]
    scale = np.float32(2.0 / W)
    got = np.stack([np.abs(a + np.conj(b)) * np.float32(0.5), np.abs(a - np.conj(b)) * np.float32(0.5)], 1) * scale
    return mags_error(got, es.truth_frame(lr, W), floor)
