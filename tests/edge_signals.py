"""Edge-of-frame streams for every transform route (a plain helper of tests/test_edge_signals.py and tests/test_gpu_edges.py).

Windowed white noise hides a misread at the first and last samples of a frame: the periodic Hann window weights sample n by
sin^2(pi n / W), so a wrong value there barely moves the magnitudes.  The streams built here are zero except for impulse pairs whose
WINDOWED values are about +-1 wherever they sit, so that dropping an edge sample, reading it at the wrong weight, at the wrong position
or from the wrong channel moves the error by orders of magnitude (tests/test_edge_signals.py proves it on the float64 truth).

ROUTES is the route table: one row per transform route, with the kernel and render_path bits the GPU test asserts before anything else,
so that a change in dispatch cannot silently move a row onto another kernel.  build_stream() lays out the stream of a row."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import oracle
from conftest import FLOOR_K16, FLOOR_WIDE, PEAK_FLOOR, REL_TOL

SR = 48000.0
SENTINEL = np.float32(1e12)   # on the offsets where the reference's float32 window is exactly 0 (see build_stream)
N_TARGET_EDGE = 8             # first / last non-zero-weight offsets of every frame that are targets


@dataclass(frozen=True)
class Route:
    name: str
    W: int
    H: int
    channels: int
    flags: tuple = ()              # SpectrogramEngine keyword flags set to True
    kernel: int = 0                # expected info.stft_kernel
    bits_set: int = 0              # render_path bits that must be set ...
    bits_clear: int = 0            # ... and clear
    floor: float = FLOOR_WIDE      # the conftest floor the existing tests use for this kernel
    bands_fused: int | None = None  # expected sgx_bands_fused (None: not pinned)
    structure: tuple = ()          # structural offset families: "k1", "real", "k16", "large"
    min_frames: int = 0            # at least this many frames (kernel-11 chunk rows)
    chunk_targets: bool = False    # targets on both sides of every kernel-11 scratch-chunk boundary
    align4: bool = False           # the stream starts at a 4- but not 8-byte aligned address

    @property
    def paired(self) -> bool:
        return "paired_frames" in self.flags and self.channels == 1

    @property
    def pairs(self) -> int:
        return 1 if self.channels == 1 else self.channels // 2

    def engine_kwargs(self) -> dict:
        kw = dict(window_samples=self.W, hop_samples=self.H, channels=self.channels)
        kw.update({f: True for f in self.flags})
        return kw


R1, R2, R4, R8 = 1, 2, 4, 8   # render_path bits: fused pixels, seeded LUT index, compile-time composite-radix plan, real-input mode


def _r(name, W, H, ch, flags=(), **kw):
    return Route(name, W, H, ch, tuple(flags), **kw)


ROUTES = [
    # K1R: the real-input 4096-point kernel (sample pairs (2n, 2n + 1) as one complex value); H 256 slides a register window
    _r("k1r_h256", 2048, 256, 1, kernel=2, bits_set=R8, floor=PEAK_FLOOR, structure=("k1", "real")),
    _r("k1r_h100", 2048, 100, 1, kernel=2, bits_set=R8, floor=PEAK_FLOOR, structure=("k1", "real")),
    # (a stream 4- but not 8-byte aligned: the same context, the (s, s) kernel takes it -- tests/test_gpu_parity.py)
    _r("k1r_h256_align4", 2048, 256, 1, kernel=2, bits_set=R8, floor=PEAK_FLOOR, structure=("k1", "real"), align4=True),
    # K1: the 4096-point kernel on (l, r), on (s, s), on frame pairs, on de-interleaved channel pairs
    _r("k1_lr_h256", 2048, 256, 2, kernel=2, bits_clear=R8, floor=PEAK_FLOOR, structure=("k1",)),
    _r("k1_lr_h58", 2048, 58, 2, kernel=2, bits_clear=R8, floor=PEAK_FLOOR, structure=("k1",)),
    _r("k1_complex_mono", 2048, 256, 1, ("complex_mono",), kernel=2, bits_clear=R8, floor=PEAK_FLOOR, structure=("k1",)),
    _r("k1_paired_mono", 2048, 256, 1, ("paired_frames",), kernel=2, bits_clear=R8, floor=PEAK_FLOOR, structure=("k1",)),
    _r("k1_ch4", 2048, 256, 4, kernel=2, bits_clear=R8, floor=FLOOR_WIDE, structure=("k1",)),
    _r("k1_ch8", 2048, 256, 8, kernel=2, bits_clear=R8, floor=FLOOR_WIDE, structure=("k1",)),
    # K16: the 16384-point kernel (row pairs when H is a multiple of 512; mono on a duplicated plane)
    _r("k16_lr_h512", 8192, 512, 2, kernel=10, floor=FLOOR_K16, structure=("k16",)),
    _r("k16_lr_h300", 8192, 300, 2, kernel=10, floor=FLOOR_K16, structure=("k16",)),
    _r("k16_ch8_h512", 8192, 512, 8, kernel=10, floor=FLOOR_K16, structure=("k16",)),
    _r("k16_ch8_h300", 8192, 300, 8, kernel=10, floor=FLOOR_K16, structure=("k16",)),
    _r("k16_mono_h512", 8192, 512, 1, kernel=10, floor=FLOOR_K16, structure=("k16",)),
    # K48: the 4800-point kernel
    _r("k48_lr", 2400, 93, 2, kernel=9, bits_clear=R8, floor=FLOOR_WIDE, bands_fused=0),
    _r("k48_paired_mono", 2400, 93, 1, ("paired_frames",), kernel=9, bits_clear=R8, floor=FLOOR_WIDE),
    # mixed radix: compile-time plans (bit 2), real-input mode (bit 3, two frames per workgroup), run-time geometry (bit 2 clear).
    # Every W 2400 context reports stft_kernel 9 (w4800_supported looks only at W); mono and 4 channels run the mixed-radix kernel,
    # pinned here by the render_path bits and bands_fused.
    _r("mixed_w2205_real", 2205, 551, 1, kernel=6, bits_set=R4 | R8, bands_fused=1, structure=("real",)),
    _r("mixed_w2400_generic", 2400, 93, 2, ("mixed_generic",), kernel=6, bits_set=R4, bits_clear=R8),
    _r("mixed_w2400_real", 2400, 93, 1, kernel=9, bits_set=R4 | R8, bands_fused=1, structure=("real",)),
    _r("mixed_w2400_ch4", 2400, 93, 4, kernel=9, bits_set=R4, bits_clear=R8, bands_fused=1),
    _r("mixed_w1024_lr", 1024, 100, 2, kernel=6, bits_set=R4, bits_clear=R8),
    _r("mixed_w1024_real", 1024, 100, 1, kernel=6, bits_set=R4 | R8, structure=("real",)),
    _r("mixed_w4096_lr", 4096, 1000, 2, kernel=6, bits_set=R4, bits_clear=R8),
    _r("mixed_w4096_real", 4096, 1000, 1, kernel=6, bits_set=R4 | R8, structure=("real",)),
    # (2W = 1470 and 10000 both lie on the run-time geometry: neither has a compile-time plan, MIX_FIXED_PLANS / MIX_FIXED4_PLANS)
    _r("mixed_w735_runtime_lr", 735, 200, 2, kernel=6, bits_clear=R4 | R8),
    _r("mixed_w5000_runtime_real", 5000, 1250, 1, kernel=6, bits_set=R8, bits_clear=R4, structure=("real",)),
    # chirp-z through the composite-radix stages (kernel 4, bit 2)
    _r("chirpz_w1102_real", 1102, 275, 1, kernel=4, bits_set=R4 | R8, structure=("real",)),
    _r("chirpz_w1102_lr", 1102, 275, 2, kernel=4, bits_set=R4, bits_clear=R8),
    _r("chirpz_w1852_lr", 1852, 463, 2, kernel=4, bits_set=R4, bits_clear=R8),
    # the radix-4 Bluestein ladder (kernel 4, bit 2 clear)
    _r("bluestein_w1102", 1102, 275, 2, ("force_generic",), kernel=4, bits_clear=R4 | R8),
    _r("bluestein_w23", 23, 5, 2, kernel=4, bits_clear=R4 | R8),
    # the generic power-of-two kernel
    _r("generic_w64_mono", 64, 16, 1, kernel=0, bits_clear=R4 | R8),
    _r("generic_w64_lr", 64, 16, 2, kernel=0, bits_clear=R4 | R8),
    _r("generic_w256_mono", 256, 60, 1, kernel=0, bits_clear=R4 | R8),
    _r("generic_w256_lr", 256, 60, 2, kernel=0, bits_clear=R4 | R8),
    _r("generic_w2048_mono", 2048, 256, 1, ("force_generic",), kernel=0, bits_clear=R4 | R8, floor=PEAK_FLOOR),
    _r("generic_w2048_lr", 2048, 256, 2, ("force_generic",), kernel=0, bits_clear=R4 | R8, floor=PEAK_FLOOR),
    # kernel 11 (SGX_FLAG_LARGE_TRANSFORM): direct plans, chirp-z plans, and batches that cross scratch-chunk boundaries
    _r("large_w10290_mono", 10290, 5148, 1, ("large_transforms",), kernel=11, structure=("large",)),
    _r("large_w16384_lr", 16384, 8195, 2, ("large_transforms",), kernel=11, structure=("large",)),
    _r("large_w19200_lr", 19200, 4800, 2, ("large_transforms",), kernel=11, structure=("large",)),
    _r("large_w1m_lr", 1 << 20, 1 << 20, 2, ("large_transforms",), kernel=11, structure=("large",)),
    _r("large_w6001_chirp_lr", 6001, 3003, 2, ("large_transforms",), kernel=11, structure=("large",)),
    _r("large_w65537_chirp_lr", 65537, 32771, 2, ("large_transforms",), kernel=11, structure=("large",)),
    _r("large_w6001_chunks", 6001, 6001, 2, ("large_transforms",), kernel=11, structure=("large",), min_frames=300, chunk_targets=True),
    _r("large_w16384_ch4_chunks", 16384, 16384, 4, ("large_transforms",), kernel=11, structure=("large",), min_frames=70,
       chunk_targets=True),
]
ROUTE = {r.name: r for r in ROUTES}
assert len(ROUTE) == len(ROUTES)


# ---- the multi-pass transform's plan (a restatement of large_plan.hpp: make_plan, scratch_per_transform) and chunking -----------
LARGE_MAX_SUB = 4096
LARGE_SCRATCH_BYTES = 64 << 20


def _smooth7(n: int) -> bool:
    for f in (2, 3, 5, 7):
        while n % f == 0:
            n //= f
    return n == 1


def large_plan(W: int):
    """(L, N1, N2, chirp) of make_plan: 2W smooth -> P = N1 x N2, N1 the largest divisor <= sqrt(P) with P / N1 <= 4096;
    otherwise chirp-z over L = pow2 >= 3W - 1, N1 = 2^floor(log2(L) / 2)"""
    P = 2 * W
    if _smooth7(P):
        N1 = max(d for d in range(1, int(np.sqrt(P)) + 2) if d * d <= P and P % d == 0 and P // d <= LARGE_MAX_SUB)
        return P, N1, P // N1, False
    L = 1
    while L < 3 * W - 1:
        L <<= 1
    N1 = 1 << ((L.bit_length() - 1) // 2)
    return L, N1, L // N1, True


def large_chunk(W: int) -> int:
    """transforms per chunk (stft_large.hip: large_init): kScratchBytes / scratch_per_transform, clamped to 1 .. 65535"""
    L, _, _, chirp = large_plan(W)
    per = L * 8 * (1 if chirp else 2)
    return min(max(LARGE_SCRATCH_BYTES // per, 1), 65535)


def chunk_boundary_frames(W: int, pairs: int, frames: int) -> list:
    """frames on both sides of every chunk boundary of a full run (launch_large: transforms frame-major, pair-minor)"""
    chunk = large_chunk(W)
    out = set()
    for t in range(chunk, frames * pairs, chunk):
        out.update(((t - 1) // pairs, t // pairs))
    return sorted(out)


# ---- target offsets ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hann(W: int) -> np.ndarray:
    w = oracle.hann_window(W)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def zero_offsets(W: int) -> tuple:
    """Z: the offsets where the reference's float32 window is exactly 0 (offset 0 always; more at W >= 65536)"""
    return tuple(int(i) for i in np.flatnonzero(hann(W) == 0))


def structural_offsets(route: Route) -> list:
    W = route.W
    out = []
    if "k1" in route.structure:        # K1 / K1R: 256-sample rows (and K1R's sliding register window)
        out += [m + d for m in range(256, W, 256) for d in (-1, 1)]
    if "k16" in route.structure:       # K16: row pairs of 512 samples
        out += [m + d for m in range(512, W, 512) for d in (-1, 1)]
    if "real" in route.structure:      # real-input modes: sample pairs (2j, 2j + 1), both halves, away from the ends too
        for e in (2, 2 * (W // 6), 2 * (W // 4) - 2, 2 * (W // 4), W - 4 - (W % 2)):
            out += [e, e + 1]
    if "large" in route.structure:     # kernel 11: the column x[N2 n1 + n2] of each n2 crosses W (n >= W is not read)
        _, N1, N2, _ = large_plan(W)
        r = (W - 1) // N2 * N2          # the first offset of the last (partial or whole) row of columns inside the window
        for base in (N2, r, W - N2):
            out += [base - 1, base, base + 1]
    return out


def target_offsets(route: Route) -> list:
    """E: the first and last N_TARGET_EDGE offsets of non-zero weight, W / 2, and the row's structural offsets"""
    W = route.W
    Z = set(zero_offsets(W))
    live = [n for n in range(W) if n not in Z]
    E = live[:N_TARGET_EDGE] + live[-N_TARGET_EDGE:] + [W // 2] + structural_offsets(route)
    seen, out = set(), []
    for n in E:
        if 0 < n < W and n not in Z and n not in seen:
            seen.add(n)
            out.append(n)
    return out


# ---- the stream ------------------------------------------------------------------------------------------------------------------
@dataclass
class Slot:
    frame: int
    kind: str              # "target": one impulse pair; "sentinel": a pair plus SENTINEL on every offset of Z; "empty"
    n: int = -1            # target offset
    m: int = -1            # partner offset
    channel: int = 0


@dataclass
class EdgeStream:
    route: Route
    pcm: np.ndarray        # [samples][channels] float32
    frames: int
    E: list
    slots: list = field(default_factory=list)

    @property
    def Z(self):
        return zero_offsets(self.route.W)

    def frame(self, t: int) -> np.ndarray:
        """[W][channels] samples of frame t"""
        H, W = self.route.H, self.route.W
        return self.pcm[t * H:t * H + W]

    def target_slots(self):
        return [s for s in self.slots if s.kind == "target"]


def _amp(W: int, n: int, sign: float) -> np.float32:
    """+-1 / hann[n] in float32: the windowed value is about +-1 wherever n sits"""
    return np.float32(sign) / hann(W)[n]


def _sequence(route: Route, E: list):
    seq = [("target", n) for n in E]
    if route.paired:   # frame pairs (2q, 2q + 1): every target once in an even and once in an odd frame (slot parity = frame parity)
        if len(E) % 2 == 0:
            seq.append(("empty", -1))
        seq += [("target", n) for n in E]
    # sentinel frames between empty ones: their samples leak into the neighbouring frames at full weight, never into a target's partner
    seq += [("empty", -1), ("sentinel", -1), ("empty", -1), ("sentinel", -1), ("empty", -1)]
    return seq


def build_stream(route: Route, E: list | None = None, seed: int = 0) -> EdgeStream:
    """The PCM stream of a row for target offsets E (default target_offsets(route)).

    Target frames lie ceil(W / H) frames (rounded up to odd, so that their parity alternates) apart: their windows are disjoint, so the
    window of each holds exactly its own two samples, on one channel.  Sentinel frames also hold SENTINEL on every offset of Z (on
    every channel): the reference multiplies them by an exact 0.  Empty slots hold nothing.  The first and the last frame are targets,
    and the stream ends with the last frame's last sample."""
    W, H, C = route.W, route.H, route.channels
    E = target_offsets(route) if E is None else list(E)
    rng = np.random.default_rng([seed, W, H, C, sum(map(ord, route.name))])
    step = -(-W // H)
    if step > 1 and step % 2 == 0:
        step += 1
    if route.chunk_targets:
        assert step == 1, "chunk-boundary targets need H >= W (adjacent frames both targets)"
    seq = _sequence(route, E)
    k = 0
    while len(seq) < route.min_frames - 1:       # (chunk rows: every further frame a target, cycling through E)
        seq.append(("target", E[k % len(E)]))
        k += 1
    seq.append(("target", max(E)))                # the last frame: a target, its sample at the last offset of non-zero weight
    frames = (len(seq) - 1) * step + 1
    pcm = np.zeros(((frames - 1) * H + W, C), np.float32)
    Z = zero_offsets(W)
    Zs = set(Z)
    live = np.array([i for i in range(W) if i not in Zs])
    slots = []
    for k, (kind, n) in enumerate(seq):
        t = k * step
        if kind == "empty":
            slots.append(Slot(t, kind))
            continue
        if kind == "sentinel":
            n = int(rng.choice(live))
        while True:
            m = int(rng.choice(live))
            if abs(m - n) >= 2:
                break
        ch = k % C
        base = t * H
        pcm[base + n, ch] = _amp(W, n, rng.choice([-1.0, 1.0]))
        pcm[base + m, ch] = _amp(W, m, rng.choice([-1.0, 1.0]))
        if kind == "sentinel":
            for j, z in enumerate(Z):
                for c in range(C):
                    pcm[base + z, c] = SENTINEL if (j + c) % 2 == 0 else -SENTINEL
        slots.append(Slot(t, kind, n, m, ch))
    return EdgeStream(route, pcm, frames, E, slots)


# ---- the float64 truth ----------------------------------------------------------------------------------------------------------
def frame_lr(x: np.ndarray, pair: int) -> np.ndarray:
    """[W][channels] -> the (l, r) input of one transform: (s, s) for mono, channels (2 pair, 2 pair + 1) otherwise"""
    return np.stack([x[:, 0], x[:, 0]], 1) if x.shape[1] == 1 else x[:, 2 * pair:2 * pair + 2]


def truth_frame(lr: np.ndarray, W: int, win: np.ndarray | None = None) -> np.ndarray:
    """oracle.np_truth_frame (bit for bit) with the window as an argument: [W - 1][2] float64"""
    win = hann(W) if win is None else win
    lr = np.ascontiguousarray(lr, np.float32).reshape(-1, 2)[:W]
    zl, zr = lr[:, 0] * win, lr[:, 1] * win
    if not zl.any() and not zr.any():
        return np.zeros((W - 1, 2))
    z = zl.astype(np.float64) + 1j * zr.astype(np.float64)
    P = 2 * W
    F = np.fft.fft(np.concatenate([z, np.zeros(W, np.complex128)]))
    k = np.arange(1, W)
    a, b = F[k], F[P - k]
    left = np.abs(a + np.conj(b)) / 2.0
    right = np.abs(a - np.conj(b)) / 2.0
    return np.stack([left, right], axis=1) * (2.0 / W)


def windowed_silent(x: np.ndarray, W: int) -> np.ndarray:
    """per channel: does the frame [W][channels] hold no non-zero windowed sample?"""
    return ~((x * hann(W)[:, None]) != 0).any(axis=0)


def pair_error(x, ref, floor, partner_peak):
    """mags_error with the larger of the frame's own and its partner frame's peak (paired mono frames share one transform)"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    peak = max(float(np.abs(ref).max()), partner_peak)
    allow = np.maximum(REL_TOL * np.maximum(np.abs(ref), floor * peak), 1e-30)
    return float((np.abs(x - ref) / allow).max())
