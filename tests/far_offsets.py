"""Where a call's offsets pass 2^31 and 2^32: the case tables and the arithmetic of tests/test_gpu_far_offsets.py (a plain helper: no GPU,
no torch at import time; tests/test_far_offsets.py checks it).

Every kernel does its own address arithmetic, and an offset truncated to 32 bits wraps to a LOWER, valid address of the same buffer:
nothing faults, the call returns the rows of other samples.  So the streams here live in arenas that hold the quiet NaN of
bounds_arena.NAN_WORD in every word but the samples the frames of one call own: a read at a wrapped offset returns NaN, not a plausible
zero (read_model() shows it on one address computation).  The marks:
  bytes from the buffer's base     2^31 and 2^32                           (arena A: 2^30 floats + 64 MiB)
  32-bit words from the base       2^31 and 2^32, bytes 2^33 and 2^34      (arena B: 2^32 floats + 64 MiB)
  the frame index                  2^31 and 2^32, reachable at H = 1 only  (arena B)
  the hop itself                   H C 4 bytes on either side of 2^31 and 2^32 (two frames from arena A, three from arena B)
A mark is crossed when it lies inside the window of a frame the call reads (an output: inside a row the call writes) and the frame or
row before it and the one after it belong to the same call."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np

import bounds_arena as ba
import edge_signals as es
from conftest import FLOOR_K16

SLACK_BYTES = 64 << 20
ARENA_FLOATS = {"A": (1 << 30) + SLACK_BYTES // 4, "B": (1 << 32) + SLACK_BYTES // 4}
ARENA_B_HEADROOM = 8 << 30     # arena B's cases may skip only where less than the arena plus this is free
CASE_CAP_BYTES = 12 << 30      # input plus output of one case of part 4
PIECE_LIMIT = 1 << 31          # every piece of a checksum stays below this many bytes
FRAMES_PER_CALL = 5
NOISE_SEED = 0x5EED0C00

# (arena, what, float index from the stream's base)
INPUT_MARKS = [("A", "byte 2^31", 1 << 29), ("A", "byte 2^32", 1 << 30), ("B", "word 2^31", 1 << 31), ("B", "word 2^32", 1 << 32)]
OUTPUT_MARKS = [1 << 31, 1 << 32]   # bytes from the output's base


def arena_bytes(arena: str) -> int:
    return ARENA_FLOATS[arena] * 4


# ---- the kernel families: one row of edge_signals.ROUTES each -----------------------------------------------------------------------
# (the 16384-point kernel on frame pairs of a mono stream has no row there: test_gpu_parity.py runs it; the row is stated here)
K16_PAIRED = es.Route("k16_paired_mono", 8192, 512, 1, ("paired_frames",), kernel=10, floor=FLOOR_K16, structure=("k16",))
FAMILIES = {
    "k1r": "k1r_h256", "k1_lr": "k1_lr_h256", "k1_paired": "k1_paired_mono", "k48_lr": "k48_lr", "k48_paired": "k48_paired_mono",
    "mixed_fixed": "mixed_w1024_lr", "mixed_real": "mixed_w2205_real", "mixed_runtime": "mixed_w735_runtime_lr",
    "mixed_runtime_real": "mixed_w5000_runtime_real", "chirpz": "chirpz_w1102_lr", "bluestein": "bluestein_w1102",
    "generic": "generic_w256_mono", "k16_lr": "k16_lr_h300", "k16_mono": "k16_mono_h512", "k16_paired": "k16_paired_mono",
    "large_direct": "large_w19200_lr", "large_chirp": "large_w6001_chirp_lr",
}


# (nor have the Bluestein ladder and kernel 11's chirp plan on a mono stream: part 3 takes them around frame 2^32, which no (l, r) stream
# of arena B reaches)
BLUESTEIN_MONO = es.Route("bluestein_w1102_mono", 1102, 275, 1, ("force_generic",), kernel=4, bits_clear=es.R4 | es.R8)
LARGE_CHIRP_MONO = es.Route("large_w6001_chirp_mono", 6001, 3003, 1, ("large_transforms",), kernel=11, structure=("large",))
OWN_ROWS = {r.name: r for r in (K16_PAIRED, BLUESTEIN_MONO, LARGE_CHIRP_MONO)}


def route(name: str) -> es.Route:
    return OWN_ROWS[name] if name in OWN_ROWS else es.ROUTE[name]


def family_route(family: str) -> es.Route:
    return route(FAMILIES[family])


def base_offset(r: es.Route) -> int:
    """floats between the arena's first word and the stream's base: 1 on the align4 row (a mono stream 4 but not 8 bytes aligned)"""
    return 1 if r.align4 else 0


def stream_samples(r: es.Route, arena: str) -> int:
    """the samples of the whole arena as one stream"""
    return (ARENA_FLOATS[arena] - base_offset(r)) // r.channels


def window(r: es.Route, t: int):
    """[lo, hi): the float indices (from the stream's base) of frame t's window"""
    return t * r.H * r.channels, (t * r.H + r.W) * r.channels


def last_whole_frame_end(r: es.Route, n_samples: int) -> int:
    total = (n_samples - r.W) // r.H + 1 if n_samples >= r.W else 0
    return (total - 1) * r.H + r.W if total else 0


def owned(r: es.Route, first: int, n: int, n_samples: int):
    """[lo, hi): the samples a call owns (bounds_arena.needed_samples: a paired row's partner frames included), clipped to the last
    whole frame of a stream of n_samples -- a partner the stream does not hold has no samples"""
    lo, hi = ba.needed_samples(r, first, n)
    return lo, min(hi, last_whole_frame_end(r, n_samples))


def owned_windows(r: es.Route, first: int, n: int, n_samples: int):
    """the same as one [lo, hi) per frame (hops beyond the window: the gaps between the windows stay NaN)"""
    end = first + n
    if r.paired:
        first -= first % 2
        end += end % 2
    total = (n_samples - r.W) // r.H + 1
    return [(t * r.H, t * r.H + r.W) for t in range(first, min(end, total))]


# ---- parts 1 and 3: a mark inside frame f0 + 2 of two calls of five frames ----------------------------------------------------------
@dataclass(frozen=True)
class InputCase:
    part: int
    row: str            # the row of ROUTES (part 3: the row whose W, channels and flags the H = 1 context takes)
    route: es.Route
    arena: str
    what: str
    mark: int           # float index from the stream's base
    f0: int

    @property
    def id(self):
        return f"{self.row}-{self.what.replace(' ', '_')}"

    def calls(self):
        """(first_frame, frames, n_samples): one call says the stream ends with its last frame, the other hands over the whole arena and
        lets max_frames do the limiting; first_frame f0 and f0 + 1 cover both parities"""
        r, n = self.route, FRAMES_PER_CALL
        return [(self.f0, n, (self.f0 + n - 1) * r.H + r.W), (self.f0 + 1, n, stream_samples(r, self.arena))]


def place_f0(r: es.Route, mark: int) -> int:
    """f0 such that float index `mark` lies inside the window of frame f0 + 2, the last frame that starts at or below it: frames f0 + 3
    and f0 + 4 START beyond the mark (a truncated frame offset), the windows that straddle it cross it lane by lane (a truncated sum of
    frame and lane offset)"""
    t = mark // (r.H * r.channels)
    lo, hi = window(r, t)
    assert lo <= mark < hi, (r.name, mark, "the mark lies in a gap between two frames")
    return t - 2


def input_cases():
    """part 1: every row of ROUTES at every mark"""
    return [InputCase(1, r.name, r, arena, what, mark, place_f0(r, mark)) for r in es.ROUTES for arena, what, mark in INPUT_MARKS]


# part 3: one H = 1 context per kernel family on arena B.  Mono rows (paired where the family pairs frames) around frames 2^31 and 2^32,
# (l, r) rows around frame 2^31 = float index 2^32.  Every family has a mono context: a frame index truncated to 32 bits shows at frame
# 2^32 only.  The (l, r) rows add the two-channel form of the families that have one.
INDEX_MONO_ROWS = ["k1r_h256", "k1_complex_mono", "k1_paired_mono", "k48_paired_mono", "mixed_w2205_real", "mixed_w1024_real",
                   "mixed_w5000_runtime_real", "chirpz_w1102_real", "generic_w256_mono", "k16_mono_h512", "k16_paired_mono",
                   "large_w10290_mono", "bluestein_w1102_mono", "large_w6001_chirp_mono"]
INDEX_LR_ROWS = ["k1_lr_h256", "k48_lr", "mixed_w1024_lr", "mixed_w735_runtime_lr", "chirpz_w1102_lr", "bluestein_w1102",
                 "generic_w256_lr", "k16_lr_h300", "large_w19200_lr", "large_w6001_chirp_lr"]


def index_cases():
    out = []
    for name in INDEX_MONO_ROWS + INDEX_LR_ROWS:
        r = dataclasses.replace(route(name), H=1)
        for fm in ((1 << 31, 1 << 32) if r.channels == 1 else (1 << 31,)):
            what = f"frame 2^{fm.bit_length() - 1}"
            out.append(InputCase(3, name, r, "B", what, fm * r.channels, fm - 2))
    return out


# ---- the compact replay -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Replay:
    shift: int        # samples: replay sample s is arena sample s + shift; a whole even number of frames
    first: int        # first_frame of the replay: 0 or 1, the call's parity
    lo: int           # [lo, hi): the owned samples, replay indices
    hi: int

    @property
    def n_samples(self):
        return self.hi


def replay_of(r: es.Route, first: int, lo: int, hi: int) -> Replay:
    even = first - first % 2
    shift = even * r.H
    assert lo >= shift
    return Replay(shift, first - even, lo - shift, hi - shift)


def replay_pad(src_addr: int, dst_addr: int) -> int:
    """floats to skip at the head of a fresh tensor at dst_addr so that its samples sit at src_addr modulo 16"""
    assert (src_addr - dst_addr) % 4 == 0
    return (src_addr - dst_addr) % 16 // 4


# ---- part 2: the hop as the large number -----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HopCase:
    family: str
    route: es.Route     # the family's row with the large hop
    small: es.Route     # the family's row as ROUTES has it: the replay's context
    arena: str
    what: str

    @property
    def id(self):
        return f"{self.family}-{self.arena}-{self.what.replace(' ', '_')}"

    def calls(self):
        """(first_frame, frames, n_samples): arena A frames 0 and 1; arena B frames 0, 1, 2 (the stream ends with frame 2) and the
        sub-range from frame 1 of the whole arena"""
        r = self.route
        if self.arena == "A":
            return [(0, 2, r.H + r.W)]
        return [(0, 3, 2 * r.H + r.W), (1, 2, stream_samples(r, "B"))]


def hop_values(channels: int):
    """(H, what): H C 4 bytes just below and just above 2^31 and 2^32"""
    out = []
    for e in (31, 32):
        h = (1 << e) // (4 * channels)
        out += [(h - 1, f"below 2^{e}"), (h + 1, f"above 2^{e}")]
    return out


def hop_cases():
    out = []
    for fam in FAMILIES:
        small = family_route(fam)
        for H, what in hop_values(small.channels):
            for arena in "AB":
                out.append(HopCase(fam, dataclasses.replace(small, H=H), small, arena, what))
    return out


# ---- part 4: outputs past 2^31 and 2^32 bytes --------------------------------------------------------------------------------------------
OUTPUT_KINDS = ["stft", "f16", "complex", "render", "bands", "peak_2", "fbank", "fbank_cross", "psd_1", "csd_1"]
OUTPUT_FAMILIES = [f for f in FAMILIES if f != "mixed_runtime_real"]   # (its run-time geometry and real-input mode: mixed_runtime, mixed_real)
ROWS_DEFAULT, ROWS_MAX = 1024, 65536
# the filterbank calls: the fused route (the 4096-point kernel on (l, r)) and one workspace family with a short hop.  The bank is the
# largest the fused route takes, 1024 filters (include/sgx.h: sgx_fbank_fused), of one bin each: 8 KiB and 16 KiB of sums per frame, the
# most a frame of input can be made to write -- nothing smaller crosses the marks.
BANK_KINDS = ("fbank", "fbank_cross")
BANK_OUTPUT_FAMILIES = ("k1_lr", "k48_lr")
BANK_FILTERS = 1024


def far_bank(M: int):
    """(first, count, weights): 1024 filters of one bin each, scattered over the M bins (bin 0 and bin M - 1 among them), weights of both
    signs with magnitudes in [2^-6, 1]"""
    rng = np.random.default_rng([0xFA2, M])
    first = (np.arange(BANK_FILTERS, dtype=np.int64) * 2039 % M).astype(np.uint32)
    first[1] = M - 1
    weights = (np.exp2(rng.uniform(-6.0, 0.0, BANK_FILTERS)) * rng.choice([-1.0, 1.0], BANK_FILTERS)).astype(np.float32)
    return first, np.ones(BANK_FILTERS, np.uint32), weights


def out_row_bytes(r: es.Route, kind: str, R: int) -> int:
    if kind in WELCH_KINDS:
        return welch_out_row_bytes(r, kind)
    if kind in BANK_KINDS:
        return r.pairs * BANK_FILTERS * (8 if kind == "fbank" else 16)
    if kind in ("stft", "f16", "complex"):
        return r.pairs * (r.W - 1) * {"stft": 8, "f16": 4, "complex": 16}[kind]
    return r.pairs * R * (4 if kind == "render" else 8)


@dataclass(frozen=True)
class OutputCase:
    family: str
    route: es.Route
    kind: str
    R: int
    rows: int           # output rows: frames, or peak columns of two frames
    row_bytes: int

    @property
    def id(self):
        return f"{self.family}-{self.kind}"

    @property
    def group(self):
        return 2 if self.kind == "peak_2" else 1

    @property
    def frames(self):
        return self.rows * self.group

    @property
    def n_samples(self):
        return (self.frames - 1) * self.route.H + self.route.W

    @property
    def input_bytes(self):
        return self.n_samples * self.route.channels * 4

    @property
    def output_bytes(self):
        return self.rows * self.row_bytes

    def probes(self):
        """the row holding each mark, its two neighbours, row 0 and the last row"""
        out = {0, self.rows - 1}
        for m in OUTPUT_MARKS:
            k = m // self.row_bytes
            out.update((k - 1, k, k + 1))
        return sorted(out)

    def pieces(self):
        """[(first row, rows)]: the call in pieces below PIECE_LIMIT bytes each"""
        per = (PIECE_LIMIT - 1) // self.row_bytes
        return [(a, min(per, self.rows - a)) for a in range(0, self.rows, per)]


def rows_for(row_bytes: int) -> int:
    """ceil((2^32 + 2 rows) / row_bytes)"""
    return -(-((1 << 32) + 2 * row_bytes) // row_bytes)


def output_case(family: str, kind: str) -> OutputCase:
    """R: the default 1024 rows, where ROUTES' assertions were made -- unless the input of that many frames breaks the cap (kernel 11's
    hops of thousands of samples): then the most rows a context takes, 65536, which those contexts' two-kernel route serves alike"""
    r = family_route(family)
    for R in (ROWS_DEFAULT, ROWS_MAX):
        rb = out_row_bytes(r, kind, R)
        c = OutputCase(family, r, kind, R, rows_for(rb), rb)
        if c.input_bytes + c.output_bytes <= CASE_CAP_BYTES:
            return c
    raise AssertionError((family, kind, "no row count keeps the case under the cap"))


def output_cases():
    return [output_case(f, k) for f in OUTPUT_FAMILIES for k in OUTPUT_KINDS
            if (k not in BANK_KINDS or f in BANK_OUTPUT_FAMILIES) and (k not in WELCH_KINDS or f == WELCH_OUTPUT_FAMILIES[k])]


# ---- what the method is for: one address computation, truncated --------------------------------------------------------------------------
def read_model(owned_ranges, start: int, n: int) -> np.ndarray:
    """n floats from float index `start` of an arena that holds NaN everywhere but in owned_ranges ([lo, hi) float indices), where
    float i is the deterministic value (i mod 8191) + 1"""
    idx = start + np.arange(n, dtype=np.int64)
    inside = np.zeros(n, bool)
    for lo, hi in owned_ranges:
        inside |= (idx >= lo) & (idx < hi)
    return np.where(inside, (idx % 8191 + 1).astype(np.float64), np.nan)


def frame_offset(first_frame: int, j: int, H: int, C: int, bits: int | None = None) -> int:
    """(first_frame + j) H C, as the kernels compute it -- or truncated to `bits` bits, as a kernel must not"""
    off = (first_frame + j) * H * C
    return off if bits is None else off & ((1 << bits) - 1)


# ---- the inverse --------------------------------------------------------------------------------------------------------------------------
# one context per inverse route (stft_istft.hip: istft_route): 1 where the composite-radix stages serve 2W (2W is 2-3-5-7-smooth), 2 the
# chirp-z form.  Hops beyond the window: the frames do not overlap, every sample is one frame's or an exact zero of a gap.
INVERSE_ROWS = {"route_1": "mixed_w1024_lr", "route_2": "chirpz_w1102_lr"}
INVERSE_FAR_H = (1 << 30) + 1      # part 3: t H of frames 2 .. 5 beyond 2^31, of frames 4 and 5 beyond 2^32 (first_sample with them)
INVERSE_FAR_FRAMES = 6
INVERSE_OUT_H = (1 << 20) - 1      # part 4: frame 256 covers sample 2^28 (byte 2^31 of an (l, r) output), frame 512 sample 2^29 (byte 2^32)
INVERSE_MARGIN = 64                # samples of the gaps on either side of a probed frame


def inverse_route(which: str, H: int) -> es.Route:
    return dataclasses.replace(route(INVERSE_ROWS[which]), H=H)


def inverse_out_frames() -> int:
    return (1 << 29) // INVERSE_OUT_H + 3


def inverse_probe_frames(F: int):
    return sorted({0, F - 1, *[t + d for t in ((1 << 28) // INVERSE_OUT_H, (1 << 29) // INVERSE_OUT_H) for d in (-1, 0, 1)]})


def sample_pieces(n_samples: int, channels: int):
    """[(first sample, samples)]: an output of n_samples in pieces below PIECE_LIMIT bytes"""
    per = (PIECE_LIMIT - 1) // (channels * 4)
    return [(a, min(per, n_samples - a)) for a in range(0, n_samples, per)]


# ---- part 4, the stand-alone pixel stage: input AND output past 2^32 bytes ---------------------------------------------------------------
# One context per kernel body (sgx_kernels.hip: launch_render, launch_magnitude_in, launch_render_bands).  Rows and ranges are chosen so
# that an input column and an output column are about the same size and both buffers cross the marks together.
LDS_CAP = 160 << 10    # the launchers' min(the device's opt-in LDS, 160 KiB): on gfx950 160 KiB (the GPU test reads the device's figure)


def pixel_body(entry: str, M: int, n_samples: int, n_lut: int, lds_cap: int) -> str:
    """the kernel body a call of `entry` runs, by the launchers' own inequalities on their own quantities: the bins of a column, the
    samples of the context's row table, the palette's entries, the LDS a workgroup may ask for.  (Which of the two-pass form's colour modes
    runs hangs on a host-side proof; its LDS tail is stated for both, and the cases here lie on the same side of the cap with either.)"""
    if entry == "render_bands":
        return "render_bands_kernel"
    if entry == "magnitude_in":
        return f"magnitude_in_kernel<{'true' if (M + 1) * 8 <= lds_cap else 'false'}>"
    generic_tail = ((n_lut + 255 + 1) & ~1) * 4 + ((n_lut + 1) & ~1) * 4 + n_lut * 8 + (512 + 4) * 2
    two_pass = {M <= 10240 and (M + 1 + n_samples) * 8 + tail <= lds_cap for tail in ((256 * 8, generic_tail) if n_lut == 256 else (generic_tail,))}
    assert len(two_pass) == 1, "the colour mode decides the kernel: not a case for this table"
    if two_pass.pop():
        return "render_two_pass_kernel"
    tables = (n_lut + 255) * 4
    tables_lds = tables <= lds_cap
    staged = "true" if (M + 1) * 8 + (tables if tables_lds else 0) <= lds_cap else "false"
    return f"render_kernel<{staged}>" if tables_lds else f"render_far_tables_kernel<{staged}>"


@dataclass(frozen=True)
class PixelCase:
    name: str
    body: str            # the kernel body the context must take
    entry: str           # render_mags, magnitude_in, render_bands
    W: int
    R: int
    large: bool = False  # SGX_FLAG_LARGE_TRANSFORM: a window no in-LDS kernel serves
    n_lut: int = 256     # the palette's entries: the built-in table, or pixel_plans.ramp(n_lut)
    n_ranges: int = 64   # sgx_magnitude_in: (f0, f1) ranges per column

    @property
    def id(self):
        return self.name

    @property
    def M(self):
        return self.W - 1

    @property
    def in_col_bytes(self):
        return (self.R if self.entry == "render_bands" else self.M) * 8

    @property
    def out_col_bytes(self):
        return self.n_ranges * 8 if self.entry == "magnitude_in" else self.R * 4

    @property
    def cols(self):
        return rows_for(min(self.in_col_bytes, self.out_col_bytes))

    def probes(self):
        """the columns that hold a mark of the input or of the output, their neighbours, the first and the last"""
        out = {0, self.cols - 1}
        for m in OUTPUT_MARKS:
            for cb in (self.in_col_bytes, self.out_col_bytes):
                k = m // cb
                out.update(c for c in (k - 1, k, k + 1) if c < self.cols)
        return sorted(out)

    def pieces(self):
        """[(first column, columns)]: input and output of every piece below PIECE_LIMIT bytes"""
        per = (PIECE_LIMIT - 1) // max(self.in_col_bytes, self.out_col_bytes)
        return [(a, min(per, self.cols - a)) for a in range(0, self.cols, per)]


PIXEL_CASES = [
    PixelCase("two_pass_w64", "render_two_pass_kernel", "render_mags", 64, 126),
    # a column of more than 10240 bins leaves the two-pass form: one workgroup per column, the column staged in LDS ...
    PixelCase("staged_w10290", "render_kernel<true>", "render_mags", 10290, 20578, large=True),
    # ... or, where (M + 1) * 8 bytes and the threshold tables pass 160 KiB, read where it lies
    PixelCase("unstaged_w20481", "render_kernel<false>", "render_mags", 20481, 40960, large=True),
    # a palette of more than 40 705 entries: the tables stay in global memory
    PixelCase("far_tables_w64", "render_far_tables_kernel<true>", "render_mags", 64, 126, n_lut=40706),
    PixelCase("magnitude_in_w64", "magnitude_in_kernel<true>", "magnitude_in", 64, 126),
    PixelCase("magnitude_in_w20481", "magnitude_in_kernel<false>", "magnitude_in", 20481, 1024, large=True, n_ranges=20480),
    # (an input column is twice an output column, whatever the rows: an output past 2^32 bytes has an input past 2^33, and the two
    # together are 3 (2^32 bytes + 2 columns) -- the least such a call can be, a few KiB above the 12 GiB of the batch cases)
    PixelCase("render_bands_r128", "render_bands_kernel", "render_bands", 64, 128),
]


# ---- part 4, the filterbank stages alone: sgx_fbank_mags and sgx_fbank_cross_spec with an output past 2^32 bytes ------------------------
@dataclass(frozen=True)
class BankStageCase:
    name: str
    entry: str           # fbank_mags, fbank_cross_spec
    W: int               # the shortest columns a context of the generic kernel takes: the case is its output
    n_filters: int = BANK_FILTERS

    @property
    def id(self):
        return self.name

    @property
    def M(self):
        return self.W - 1

    @property
    def in_col_bytes(self):
        return self.M * (8 if self.entry == "fbank_mags" else 16)

    @property
    def out_col_bytes(self):
        return self.n_filters * (8 if self.entry == "fbank_mags" else 16)

    @property
    def cols(self):
        return rows_for(self.out_col_bytes)

    def probes(self):
        """the columns whose sums hold a mark of the output, their neighbours, the first and the last"""
        out = {0, self.cols - 1}
        for m in OUTPUT_MARKS:
            k = m // self.out_col_bytes
            out.update((k - 1, k, k + 1))
        return sorted(out)

    def pieces(self):
        """[(first column, columns)]: the output of every piece below PIECE_LIMIT bytes"""
        per = (PIECE_LIMIT - 1) // self.out_col_bytes
        return [(a, min(per, self.cols - a)) for a in range(0, self.cols, per)]


BANK_STAGE_CASES = [BankStageCase("fbank_mags_w64", "fbank_mags", 64), BankStageCase("fbank_cross_spec_w64", "fbank_cross_spec", 64)]


# ---- part 4, the Welch calls: sgx_psd_batch / sgx_csd_batch outputs and the stages' inputs and outputs past 2^32 bytes ------------------
# The batch calls at group 1 (a column per frame: the most a frame of input can be made to write) on the two 4096-point families: the
# real-input kernel of a mono stream, whose rows launches into the workspace take the automatic weighted deal (run_claim.hpp), and the
# (l, r) kernel for the cross means.  Every range of psd_reduce passes `first_frame + f` on, up to the call's last frame.
WELCH_KINDS = ("psd_1", "csd_1")
WELCH_OUTPUT_FAMILIES = {"psd_1": "k1r", "csd_1": "k1_lr"}


def welch_out_row_bytes(r: es.Route, kind: str) -> int:
    return r.pairs * (r.W - 1) * (8 if kind == "psd_1" else 16)


@dataclass(frozen=True)
class WelchStageCase:
    name: str
    entry: str           # psd_mags, csd_spec
    W: int               # the shortest rows a context of the generic kernel takes: the case is its offsets
    groups: tuple = (1, 2)

    @property
    def id(self):
        return self.name

    @property
    def M(self):
        return self.W - 1

    @property
    def row_bytes(self):
        """a frame's rows of the input and a column of the output alike (one pair)"""
        return self.M * (8 if self.entry == "psd_mags" else 16)

    @property
    def frames(self):
        """the input crosses 2^31 and 2^32 bytes with two rows to spare"""
        return rows_for(self.row_bytes)

    def cols(self, group: int) -> int:
        return -(-self.frames // group)

    def crossed(self, group: int):
        """(input marks, output marks) a call at `group` crosses: group 1 all four; group 2 the input's two and byte 2^31 of the output"""
        out_bytes = self.cols(group) * self.row_bytes
        return [m for m in OUTPUT_MARKS if m < self.frames * self.row_bytes], [m for m in OUTPUT_MARKS if m < out_bytes]

    def probes(self, group: int):
        """the columns that hold a mark of the output, the columns whose frames hold a mark of the input, their neighbours, the first
        and the last"""
        n = self.cols(group)
        out = {0, n - 1}
        marks_in, marks_out = self.crossed(group)
        for k in [m // self.row_bytes for m in marks_out] + [m // self.row_bytes // group for m in marks_in]:
            out.update(c for c in (k - 1, k, k + 1) if 0 <= c < n)
        return sorted(out)

    def pieces(self, group: int):
        """[(first column, columns)]: the input frames and the output columns of every piece below PIECE_LIMIT bytes"""
        per = (PIECE_LIMIT - 1) // (self.row_bytes * group)
        return [(a, min(per, self.cols(group) - a)) for a in range(0, self.cols(group), per)]


WELCH_STAGE_CASES = [WelchStageCase("psd_mags_w64", "psd_mags", 64), WelchStageCase("csd_spec_w64", "csd_spec", 64)]
