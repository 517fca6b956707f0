"""Which code the pixel stage runs for a configuration, as data (a plain helper of tests/test_pixel_plans.py and
tests/test_gpu_pixel_plans.py).

The pixel stage (log-frequency resample, dB, colour) chooses its code at run time.  The rules are restated here from the launchers --
nothing asks the library:

  launch_render (csrc/sgx_kernels.hip)   render_two_pass_kernel<KPRE, MODE, SPT, NT>: nine (NT, KPRE, SPT) shapes -- (256, 8, 12),
                                         (256, 8, 0), (256, 10, 12), (256, 10, 0), (256, 16, 0), (512, 8, 0), (512, 16, 0), (1024, 8, 0),
                                         (1024, 10, 0) -- times three colour modes; else render_kernel<STAGED> per column, its threshold
                                         tables in LDS or (palettes that no LDS holds) read where they lie
  launch_magnitude_in                    magnitude_in_kernel<STAGED>: the column in LDS up to W 20480
  launch_render_bands                    the threshold tables in LDS up to 48 KiB (12 033 palette entries)
  wg4096_init (csrc/stft4096_wg.hip)     W 2048: `fusable` (rows <= 1024, padded slots <= kMaxFusedSamples, 16-bit row words), the pad
                                         slot after every row of even count >= 4, single_rows and block_max_cnt per block of 256 rows
  mixed_can_fuse_* (csrc/stft_mixed.hip) the compile-time plans: the column and its samples on the transform's LDS image ((l, r) plan), or
                                         within 160 KiB (real-input mode), and ten bins per thread at most

LDS_CAP is gfx950's 160 KiB; the library compares with min(lds_optin, 160 KiB), which is the same number on that device.

The row table comes from oracle.bin_edges and oracle.num_samples_in.  The colour mode of a 256-entry palette hangs on two host-side proofs
(wg::seed_within_one on the LUT thresholds and on the alpha thresholds) that are not restated: a Context records which way the dB range is
EXPECTED to fall (`proof`), the GPU test reads the outcome from sgx_info.render_path bit 1 where the route shows it, and seed_margin()
computes, for the one narrow range the sweep uses, how far the float32 dB ramp strays from the seed's straight line.

sweep() builds the contexts: for every inequality of the rules a PAIR of configurations on either side of it -- found by bisection over one
public knob (f_max, rows or W), everything else fixed; the row table moves in steps, so the pair is the nearest reachable value on each
side -- or a line in DEAD saying why it cannot bind, which tests/test_pixel_plans.py proves; then a representative of every launch_render
class under three palettes, and the named extras (row counts, clamped axes, single_rows masks, palette sizes, ...)."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace

import numpy as np

import length_sweep as ls

LDS_CAP = 160 * 1024          # gfx950: the LDS of a CU, and what one workgroup may ask for (min(lds_optin, 160 KiB) in the library)
K_TCELLS = 512                # sgx_internal.hpp kTCells
SEEDED_TAIL = 256 * 8         # kMonoSeed / kStereoSeed: 256 {threshold, RGBA} words
MAX_TWO_PASS_M = 1024 * 10    # launch_render: M <= 10240 (ten bins per thread of 1024 in registers)
IN_REGS_SAMPLES = 256 * 12    # SPT: 12 samples per thread of 256
WG_MAX_ROWS = 1024            # wg4096_init: fusable needs R <= 1024
WG_MAX_SLOTS = 2302           # stft4096_wg.hpp kMaxFusedSamples = kBufComplex - kColSlots = 4352 - 2050
BANDS_TABLES_LDS = 48 * 1024  # launch_render_bands: the tables in LDS up to here
FLAG_BITS = {"force_generic", "fused_render_off", "lut_walk", "large_transforms", "paired_frames", "complex_mono", "mixed_generic"}

# threads of the compile-time mixed-radix plans (the last argument of MIX_FIXED_PLANS / MIX_FIXED4_PLANS; tests/test_pixel_plans.py holds
# these tables to the macros' text), of real-input mode to pixels (MIX_REAL_RENDER_PLANS overrides), and the plans real-input mode runs two
# frames per workgroup (MIX_REAL2_RENDER_PLANS: the only three-stage plans whose real-input bands kernel exists)
MIX_THREADS = {4800: 512, 4410: 512, 3200: 512, 1600: 512, 800: 256, 8820: 512, 2048: 256, 1024: 256, 2400: 256, 2205: 192, 4096: 256,
               512: 128, 9600: 1024, 19200: 1024, 17640: 1024, 8192: 512}
MIX_REAL_THREADS = {2400: 512, 2205: 320}
MIX_REAL2 = (2400, 2205, 4800, 4410, 4096, 1024, 512, 1600, 800, 3200, 8820)
MIX_FOUR_STAGE = (9600, 19200, 17640, 8192)


# ---- a configuration -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Palette:
    kind: str = "builtin"      # "builtin": a 256-entry table by name; "ramp": n entries made by ramp(); "scheme": a callback gradient by name
    name: str = "viridis"
    n: int = 256               # entries ("scheme": not known here -- the library counts the colour steps)
    stereo: bool = False       # the diverging branch (colorscheme.rs:63-66)

    @property
    def tag(self):
        return f"{self.name if self.kind != 'ramp' else 'ramp' + str(self.n)}{'-div' if self.stereo else ''}"


@dataclass(frozen=True)
class Config:
    W: int = 2048
    sample_rate: float = 48000.0
    rows: int = 1024
    f_min: float = 32.0
    f_max: float = 22030.0
    interp: int = 0
    min_db: float = -70.0
    max_db: float = -10.0
    lut_index_mode: int = 0
    palette: Palette = Palette()
    channels: int = 1
    flags: tuple = ()

    @property
    def M(self):
        return self.W - 1

    @property
    def sr_u32(self):
        return int(np.float32(self.sample_rate))     # `sample_rate as u32` (simple_spectrogram.rs:138)

    @property
    def H(self):
        return self.W // 3 + 1

    def engine_kwargs(self) -> dict:
        kw = dict(window_samples=self.W, hop_samples=self.H, channels=self.channels, rows=self.rows, f_min=self.f_min, f_max=self.f_max,
                  interp=self.interp, min_db=self.min_db, max_db=self.max_db, lut_index_mode=self.lut_index_mode)
        for f in self.flags:
            if f == "fused_render_off":
                kw["fused_render"] = False
            else:
                kw[f] = True
        return kw


def ramp(n: int) -> np.ndarray:
    """[n][3] uint8, every entry distinct (n <= 65536): a wrong level shows as a wrong colour, whatever the size"""
    i = np.arange(n, dtype=np.uint32)
    return np.stack([i & 0xff, (i >> 8) & 0xff, (i * 37 + 11) & 0xff], 1).astype(np.uint8)


def needs_large(W: int) -> bool:
    """sgx_create: no in-LDS kernel serves W (a power of two up to 8192, a 7-smooth 2W up to 20480, or 3W - 1 <= 16384)"""
    P = 2 * W
    return not ((ls.is_pow2(P) and P <= 16384) or (ls.smooth7(P) and P <= ls.MIX_MAX_P) or 3 * W - 1 <= ls.CHIRP_MAX_L)


# ---- the row table ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class RowTable:
    counts: tuple              # samples per row, row 0 the lowest
    n_samples: int
    padded: int                # wg4096_init's slots: one pad after every row of even count >= 4
    single_rows: int           # bit i: every row of block i (256 rows) has one sample; blocks 0 .. 3
    block_max_cnt: int         # byte i: min(255, the largest count of block i)
    max_first: int
    max_count: int


def row_counts(W, sr, rows, f_min, f_max) -> np.ndarray:
    """samples per row, by the operations of oracle.bin_edges and oracle.num_samples_in on all rows at once (the bisections evaluate
    thousands of row tables): log_unmap's doubles cast to float32, then one float32 multiplication, the clamp, one subtraction, floor, at
    least 1.  tests/test_pixel_plans.py holds the edges and the counts of every context of the sweep to the oracle's, row by row"""
    lo, hi = math.log(f_min), math.log(f_max)       # (the C library's log and exp, as the oracle calls them; double arithmetic, no FMA)
    edges = np.array([math.exp((hi - lo) * (p / rows) + lo) for p in range(rows + 1)], np.float64).astype(np.float32)
    M = W - 1
    period = np.float32(np.float32(2.0) * np.float32(M)) / np.float32(sr)
    idx = np.clip(edges * period, np.float32(0.0), np.float32(M - 1))
    d = idx[1:] - idx[:-1]
    return np.maximum(np.floor(d).astype(np.int64), 1)


@functools.lru_cache(maxsize=4096)
def _row_table(W, sr, rows, f_min, f_max) -> RowTable:
    counts = row_counts(W, sr, rows, f_min, f_max)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    single = mx = 0
    for blk in range(4):
        c = counts[256 * blk:256 * (blk + 1)]
        if len(c):
            single |= int((c == 1).all()) << blk
            mx |= min(255, int(c.max())) << (8 * blk)
    return RowTable(tuple(int(c) for c in counts), int(counts.sum()), int(counts.sum() + ((counts >= 4) & (counts % 2 == 0)).sum()), single, mx,
                    int(first.max()), int(counts.max()))


def row_table(c: Config) -> RowTable:
    return _row_table(c.W, c.sr_u32, c.rows, float(c.f_min), float(c.f_max))


# ---- launch_render ---------------------------------------------------------------------------------------------------------------------------
def generic_tail(n: int) -> int:
    """kGeneric's tables behind the column, as launch_render sizes them: both float tables, the colours, the switch points of the
    diverging branch as doubles, the balance grid"""
    return ((n + 255 + 1) & ~1) * 4 + ((n + 1) & ~1) * 4 + n * 8 + (K_TCELLS + 4) * 2


def may_seed(c: Config) -> bool:
    """the palette conditions of kMonoSeed / kStereoSeed, the two proofs aside"""
    p = c.palette
    if p.kind == "scheme" or p.n != 256 or "lut_walk" in c.flags:
        return False
    return not p.stereo or c.lut_index_mode == 0


def predicates(c: Config, seeded: bool, n_lut=None) -> dict:
    """every inequality of launch_render as the launcher evaluates it, by name (None: not evaluated on this path)"""
    t, M, n = row_table(c), c.M, c.palette.n if n_lut is None else n_lut
    lds2 = (M + 1 + t.n_samples) * 8 + (SEEDED_TAIL if seeded else generic_tail(n))
    out = {"M<=10240": M <= MAX_TWO_PASS_M, "lds2<=cap": lds2 <= LDS_CAP}
    keys = ("fit>=4", "fit>=2", "grow", "need<=8", "need<=10", "R<=1024", "samples<=3072", "samples<65536", "words<65536")
    out.update({k: None for k in keys})
    if out["M<=10240"] and out["lds2<=cap"]:
        fit = LDS_CAP // lds2
        nt = 256 if fit >= 4 else (512 if fit >= 2 else 1024)
        grow = False
        while nt < 1024 and -(-M // nt) > 16:
            nt *= 2
            grow = True
        need = -(-M // nt)
        out.update({"fit>=4": fit >= 4, "fit>=2": fit >= 2, "grow": grow, "need<=8": need <= 8, "need<=10": need <= 10 if nt != 512 else None, "nt": nt})
        if nt == 256:
            out.update({"R<=1024": c.rows <= 1024, "samples<=3072": t.n_samples <= IN_REGS_SAMPLES, "samples<65536": t.n_samples < 65536,
                        "words<65536": t.max_first < 65536 and t.max_count < 65536})
    tables = (n + 255) * 4
    out["tables<=cap"] = tables <= LDS_CAP                            # else render_far_tables_kernel: the tables take no LDS
    out["staged"] = (M + 1) * 8 + (tables if tables <= LDS_CAP else 0) <= LDS_CAP
    out["bands tables<=48K"] = bands_tables_in_lds(n)                 # launch_render_bands
    return out


def render_class(c: Config, seeded: bool, n_lut=None) -> tuple:
    """("two_pass", NT, KPRE, SPT) or ("column", staged, tables_in_lds)"""
    p = predicates(c, seeded, n_lut)
    if p["M<=10240"] and p["lds2<=cap"]:
        nt = p["nt"]
        in_regs = nt == 256 and p["samples<=3072"] and p["R<=1024"] and p["samples<65536"] and p["words<65536"]
        if nt == 256:
            return ("two_pass", 256, 8, 12 if in_regs else 0) if p["need<=8"] else ("two_pass", 256, 10, 12 if in_regs else 0) if p["need<=10"] \
                else ("two_pass", 256, 16, 0)
        if nt == 512:
            return ("two_pass", 512, 8 if p["need<=8"] else 16, 0)
        return ("two_pass", 1024, 8 if p["need<=8"] else 10, 0)
    return ("column", p["staged"], p["tables<=cap"])


TWO_PASS_SHAPES = [(256, 8, 12), (256, 8, 0), (256, 10, 12), (256, 10, 0), (256, 16, 0), (512, 8, 0), (512, 16, 0), (1024, 8, 0), (1024, 10, 0)]
ALL_CLASSES = [("two_pass",) + s for s in TWO_PASS_SHAPES] + [("column", True, True), ("column", False, True)]
FAR_CLASSES = [("column", True, False), ("column", False, False)]    # render_far_tables_kernel<STAGED>: palettes above 40 705 entries only


def magnitude_in_staged(c: Config) -> bool:
    return (c.M + 1) * 8 <= LDS_CAP


def bands_tables_in_lds(n_lut: int) -> bool:
    return (n_lut + 255) * 4 <= BANDS_TABLES_LDS


def blocks_launched(c: Config, seeded: bool, n_cu: int, n_lut=None) -> int:
    """the persistent workgroups launch_render starts for many columns: n_cu * min(per_cu, 8), per_cu as LDS and 2048 threads per CU allow
    (the launcher asks the occupancy API, which also counts registers: this is an upper estimate, good for sizing a test's buffer)"""
    cls = render_class(c, seeded, n_lut)
    if cls[0] != "two_pass":
        return n_cu * 8
    n = c.palette.n if n_lut is None else n_lut
    lds2 = (c.M + 1 + row_table(c).n_samples) * 8 + (SEEDED_TAIL if seeded else generic_tail(n))
    return n_cu * max(1, min(8, LDS_CAP // lds2, 2048 // cls[1]))


# ---- the fused routes ------------------------------------------------------------------------------------------------------------------------
def stft_kernel(c: Config):
    """sgx_create's kernel where the restatement claims it: 2 (W 2048), 6 / 9 (mixed radix); None otherwise"""
    if "large_transforms" in c.flags and needs_large(c.W):
        return 11
    if c.W == 2048 and "force_generic" not in c.flags:
        return 2
    if "force_generic" in c.flags:
        return None
    served = ls.smooth7(2 * c.W) and 2 * c.W <= ls.MIX_MAX_P and c.W not in ls.SMOOTH_EXCLUDED
    if served:
        return 9 if c.W == 2400 and "mixed_generic" not in c.flags else 6
    return None


def wg_predicates(c: Config) -> dict:
    t = row_table(c)
    return {"wg rows<=1024": c.rows <= WG_MAX_ROWS, "wg slots<=2302": t.padded <= WG_MAX_SLOTS,
            "wg words": t.max_count < 65536 and t.padded < 65536 + 1}


def wg_fusable(c: Config) -> bool:
    """wg4096_init's `fusable` (`r.count >= 65536u || samples.size() >= 65536`: the row word's 16 bits of count)"""
    return all(wg_predicates(c).values())


def fused_palette_shape(c: Config) -> bool:
    """the palette conditions every fused PCM-to-pixels kernel shares, the seed proof aside: a sequential 256-entry table"""
    p = c.palette
    return p.kind != "scheme" and p.n == 256 and not p.stereo


def mixed_real_serves(c: Config) -> bool:
    """a mono stream, every frame its own transform, and W has a plan (from W 8 on)"""
    return c.channels == 1 and c.W >= 8 and ls.mixed_radix_plan(c.W) is not None and "paired_frames" not in c.flags and "complex_mono" not in c.flags


def mixed_predicates(c: Config) -> dict:
    """the *_column_fits inequalities of the plan this context's stream runs; {} where no compile-time plan does"""
    t, W, M = row_table(c), c.W, c.M
    if mixed_real_serves(c):
        if not ls.mixed_is_fixed(W):
            return {}
        nt = MIX_REAL_THREADS.get(W, MIX_THREADS[W])
        return {"real W/2<=10nt": W // 2 <= nt * 10, "real column<=160K": (M + 1 + t.n_samples) * 8 <= LDS_CAP}
    P = 2 * W
    if not ls.mixed_is_fixed(P):
        return {}
    plan = ls.mixed_radix_plan(P)
    pad = ls.mixed_pad_every(P, plan)
    lds_points = P + P // pad if pad else P
    return {"mixed M<=10nt": M <= MIX_THREADS[P] * 10, "mixed column<=image": M + 1 + t.n_samples <= lds_points}


def mixed_column_fits(c: Config) -> bool:
    p = mixed_predicates(c)
    return bool(p) and all(p.values())


def bands_kernel_exists(fixed: int, real: bool) -> bool:
    if real and fixed in MIX_REAL2:
        return True
    return fixed in MIX_FOUR_STAGE or (not real and fixed in MIX_THREADS)


def bands_fused(c: Config):
    """sgx_bands_fused where the restatement claims it (None: it does not)"""
    k = stft_kernel(c)
    if "fused_render_off" in c.flags:
        return 0
    if k == 2:
        return int(wg_fusable(c))
    if k in (6, 9):
        if k == 9 and c.channels <= 2 and not mixed_real_serves(c):
            return 0           # rows from the tuned 4800-point kernel: the two-kernel route
        real = mixed_real_serves(c)
        return int(mixed_column_fits(c) and bands_kernel_exists(c.W if real else 2 * c.W, real))
    return 0 if k == 11 else None


def bands_peak_fused(c: Config):
    b = bands_fused(c)
    if b is None:
        return None
    return int(b == 1 and stft_kernel(c) == 2 and not (c.channels == 1 and "paired_frames" in c.flags))


def render_bits(c: Config, proof):
    """(bit 0, bit 1) of render_path where the restatement claims them, given the seed proof's outcome (None: unknown -> bit 1 not claimed)"""
    k = stft_kernel(c)
    if k is None:
        return None, None
    if "fused_render_off" in c.flags or k == 11:
        return 0, 0
    if k == 2:
        fused = wg_fusable(c) and fused_palette_shape(c)
        if not fused:
            return 0, 0
        return 1, (None if proof is None else int(proof and "lut_walk" not in c.flags))
    if not (mixed_column_fits(c) and fused_palette_shape(c)) or "lut_walk" in c.flags:
        return 0, 0
    return (None, None) if proof is None else (int(proof), int(proof))


# ---- the seed's margin -----------------------------------------------------------------------------------------------------------------------
def seed_margin(min_db: float, max_db: float, n_levels: int = 256):
    """(margin, skipped): how far, in LUT indices, the switch points of the oracle's color_for lie from the seed's straight line
    u(power) = log2(power + 1e-7) a + b (lut_seed_coefficients, the floor(t n) rule), and how many levels no power reaches.

    The switch point into level e + 1 is found by bisection over the float32 bit patterns of l (r = 0: the level is monotone in l) and the
    margin is the largest |u(l * l) - (e + 1)| over the levels that have one.  seed_within_one keeps 0.49 of an index in hand at every
    switch point.  Where a level is skipped, two neighbouring switch points coincide and u cannot be within half an index of both e + 1
    and e + 2: the proof cannot hold, whatever its own arithmetic is -- and a float32 dB ramp skips levels as soon as the span holds fewer
    float32 dB values than the palette has levels."""
    import oracle
    grad = ramp(n_levels)
    lo_db, hi_db = float(np.float32(min_db)), float(np.float32(max_db))
    a, b = 10.0 * np.log10(2.0) * n_levels / (hi_db - lo_db), -lo_db * n_levels / (hi_db - lo_db)

    def level(bits):
        l = np.uint32(bits).view(np.float32)
        rgb, _ = oracle.color_for(grad, float(l), 0.0, False, min_db, max_db, 0)
        return int(rgb[0]) | (int(rgb[1]) << 8)

    top = int(np.float32(3.0e38).view(np.uint32))
    switch = []
    for want in range(1, n_levels):
        lo, hi = 0, top
        if level(hi) < want:
            switch.append(None)          # unreachable: the library's table holds a NaN there
            continue
        while lo < hi:
            mid = (lo + hi) // 2
            if level(mid) >= want:
                hi = mid
            else:
                lo = mid + 1
        switch.append(lo)
    skipped = sum(1 for e in range(1, len(switch)) if switch[e] is not None and switch[e] == switch[e - 1]) + sum(s is None for s in switch)
    margin = 0.0
    for e, bits in enumerate(switch):
        if bits is None or bits == 0:
            continue
        l = np.uint32(bits).view(np.float32)
        power = float(np.float32(l * l) + np.float32(1e-7))
        margin = max(margin, abs(np.log2(power) * a + b - (e + 1)))
    return margin, skipped


# ---- contexts ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Context:
    name: str
    cfg: Config
    group: str                 # the chunk of the GPU sweep it runs in
    proof: object = None       # the seed proof on this dB range: True / False expected, None not claimed
    batch: bool = True         # run sgx_render_batch / sgx_bands_batch on a short stream (off for the long windows of kernel 11)
    why: str = ""

    @property
    def seeded(self) -> bool:
        return may_seed(self.cfg) and self.proof is not False

    @property
    def cls(self):
        """launch_render's class; None for a callback gradient, whose colour steps only the library counts"""
        return None if self.cfg.palette.kind == "scheme" else render_class(self.cfg, self.seeded)


@dataclass(frozen=True)
class Pair:
    target: str                # the predicate the two differ in
    a: Context                 # target holds
    b: Context                 # target fails
    knob: str
    follows: tuple = ()        # predicates that depend on the target (or are not evaluated on one side) and may differ with it


SEQ256 = Palette("builtin", "viridis", 256, False)
DIV256 = Palette("builtin", "plasma", 256, True)
RAMP7 = Palette("ramp", "ramp", 7, False)
THREE_PALETTES = (SEQ256, DIV256, RAMP7)

# inequalities that cannot bind, one line each; tests/test_pixel_plans.py proves every line
DEAD = {
    "samples<=3072": "at NT 256 the image fits four times: M + 1 + samples <= 4864; samples <= R + M - 1 and R <= 1024 give samples > 3072 only from M >= 2049, where M + 1 + 3073 > 4864",
    "samples<65536": "implied by samples <= 3072, which is evaluated first",
    "words<65536": "first and count are below the sample total, which is <= 3072 here",
    "wg words": "at M 2047 a row has at most 2046 samples, and with R <= 1024 the padded total is below 1024 + 2046 + 1024",
    "real W/2<=10nt": "every W-point plan: 4800, 4410 and 8820 / 2 <= 5120; 9600 / 2 <= 10240; 8192 is K16's; the rest are far below",
    "mixed M<=10nt": "every 2W-point plan: 19200 and 17640 / 2 - 1 <= 10240, 8820 and 8192 / 2 - 1 <= 5120, 4800 / 2 - 1 <= 2560 (256 threads: 2400 and below)",
}


def all_predicates(c: Config, seeded: bool) -> dict:
    return {**predicates(c, seeded), **(wg_predicates(c) if stft_kernel(c) == 2 else {}), **(mixed_predicates(c) if stft_kernel(c) in (6, 9) else {})}


def _flags(W, extra=()):
    return tuple(extra) + (("large_transforms",) if needs_large(W) else ())


def _with(cfg: Config, **kw) -> Config:
    """cfg with fields replaced and the flags its window needs: SGX_FLAG_LARGE_TRANSFORM where no in-LDS kernel serves W, and at W 2400 on
    (l, r) SGX_FLAG_MIXED_GENERIC -- the tuned 4800-point kernel writes rows only, so a default context's fused pixels are not those of its
    own rows (tests/test_gpu_parity.py::test_app_point_4800_point_kernel holds that route)"""
    cfg = replace(cfg, **kw)
    keep = tuple(f for f in cfg.flags if f not in ("large_transforms", "mixed_generic"))
    return replace(cfg, flags=_flags(cfg.W, keep + (("mixed_generic",) if cfg.W == 2400 and cfg.channels == 2 else ())))


def bisect(cfg: Config, knob: str, lo, hi, holds):
    """the nearest reachable values of `knob` on either side of holds(cfg): (value where it holds, value where it does not).  Integers end
    at neighbours, floats at neighbouring doubles; holds() must differ at lo and hi"""
    at = lambda v: holds(_with(cfg, **{knob: v}))   # noqa: E731
    a, b = at(lo), at(hi)
    assert a != b, (knob, lo, hi, a)
    integer = isinstance(lo, int)
    while True:
        mid = (lo + hi) // 2 if integer else lo + (hi - lo) * 0.5
        if mid == lo or mid == hi:
            break
        if at(mid) == a:
            lo = mid
        else:
            hi = mid
    return (lo, hi) if a else (hi, lo)


def _pair(target, cfg, knob, lo, hi, seeded, group, follows=(), batch=True, why="") -> Pair:
    holds = lambda c: all_predicates(c, seeded)[target]   # noqa: E731
    va, vb = bisect(cfg, knob, lo, hi, holds)
    proof = True if seeded else None
    if not group.startswith("mixed-ends"):          # a GPU case per inequality
        group += "-" + target.replace("<=", "-le-").replace(">=", "-ge-").replace("<", "-lt-").replace(" ", "-").replace("/", "")
    mk = lambda v, side: Context(f"{target} {side}: {knob} {v!r} W {cfg.W if knob != 'W' else v} ch {cfg.channels} {cfg.palette.tag}", _with(cfg, **{knob: v}), group, proof, batch, why)   # noqa: E731
    return Pair(target, mk(va, "holds"), mk(vb, "fails"), knob, tuple(follows))


NEED_FOLLOWS = ("need<=8", "need<=10", "grow", "R<=1024", "samples<=3072", "samples<65536", "words<65536", "nt")
TWO_PASS_ONLY = ("fit>=4", "fit>=2") + NEED_FOLLOWS


@functools.lru_cache(maxsize=1)
def pairs() -> tuple:
    base = Config()
    gen = replace(base, palette=RAMP7)
    narrow = dict(rows=16, f_min=100.0, f_max=200.0)
    out = []
    # --- launch_render: the two-pass form at all
    out.append(_pair("M<=10240", _with(base, rows=16, f_min=20000.0, f_max=24000.0), "W", 10241, 10242, True, "render-ends", TWO_PASS_ONLY + ("lds2<=cap",), batch=False))
    for seeded, cfg in ((True, base), (False, gen)):
        g = "render-ends" if seeded else "render-ends-generic"
        out.append(_pair("lds2<=cap", _with(cfg, W=10240), "f_max", 2000.0, 24000.0, seeded, g, TWO_PASS_ONLY))
        out.append(_pair("fit>=2", _with(cfg, W=5000), "f_max", 2000.0, 24000.0, seeded, g, NEED_FOLLOWS))
        out.append(_pair("fit>=4", _with(cfg, W=2400), "f_max", 2000.0, 24000.0, seeded, g, NEED_FOLLOWS))
    # --- bins per thread: W on either side.  Every axis here ends at Nyquist, so the top rows read the LAST bins -- the ones a prefetch of
    # too few bins per thread would leave out; the narrow axes keep the image small enough for its class
    top = dict(rows=64, f_min=20000.0, f_max=24000.0)
    out.append(_pair("need<=8", _with(base, **top), "W", 2049, 2050, True, "render-ends"))
    out.append(_pair("need<=10", _with(base, **top), "W", 2561, 2562, True, "render-ends", ("R<=1024", "samples<=3072", "samples<65536", "words<65536")))
    out.append(_pair("grow", _with(base, **top), "W", 4098, 4097, True, "render-ends", NEED_FOLLOWS + ("fit>=4", "fit>=2")))
    out.append(_pair("need<=8", _with(base, f_max=24000.0), "W", 4097, 4098, True, "render-ends"))            # NT 512
    out.append(_pair("grow", _with(base, **{**top, "rows": 256}), "W", 8194, 8193, True, "render-ends", NEED_FOLLOWS, batch=False))   # NT 512 -> 1024
    out.append(_pair("need<=8", _with(base, f_max=24000.0), "W", 8193, 8194, True, "render-ends", batch=False))   # NT 1024
    # --- the table entries in registers
    out.append(_pair("R<=1024", base, "rows", 1024, 1025, True, "render-ends", ("wg rows<=1024",)))     # (W 2048: wg4096's bound is the same)
    out.append(_pair("R<=1024", _with(gen, W=1024), "rows", 1024, 1025, False, "render-ends-generic"))
    # --- the per-column kernel and magnitude_in: the column in LDS or where it lies (kernel 11's windows)
    out.append(_pair("staged", _with(base, **narrow), "W", 20224, 20225, True, "long-windows", batch=False))
    # --- the fused 4096-point pixel path
    out.append(_pair("wg rows<=1024", replace(base, channels=2, interp=1), "rows", 1024, 1025, True, "wg-ends", ("R<=1024",)))
    out.append(_pair("wg slots<=2302", base, "f_max", 22030.0, 24000.0, True, "wg-ends"))
    out.append(_pair("wg slots<=2302", replace(base, channels=2, interp=1), "f_max", 22030.0, 24000.0, True, "wg-ends"))
    # --- the per-column kernel's threshold tables: in LDS up to 160 KiB of them (40 705 entries), read where they lie beyond
    far = lambda n: Context(f"tables<=cap {'holds' if n <= 40705 else 'fails'}: palette {n} W 2048 ch 2", Config(palette=Palette("ramp", "ramp", n, False), channels=2),   # noqa: E731
                            "palette-ends", None, False)
    # (at W 2048 the column's 16 KiB fit beside nothing: 40 705 entries run render_kernel<false>, 40 706 render_far_tables_kernel<true>)
    out.append(Pair("tables<=cap", far(40705), far(40706), "palette", ("staged", "lds2<=cap") + TWO_PASS_ONLY))
    # ... and that kernel's own staged switch, the column alone against 160 KiB
    out.append(_pair("staged", _with(Config(palette=Palette("ramp", "ramp", 65536, False), channels=2), **narrow), "W", 20480, 20481, False, "long-windows-far", batch=False))
    # --- launch_render_bands: the tables in LDS up to 48 KiB
    bt = lambda n: Context(f"bands tables<=48K {'holds' if n <= 12033 else 'fails'}: palette {n} W 2048 ch 2", Config(palette=Palette("ramp", "ramp", n, True), channels=2),   # noqa: E731
                           "palette-bands-ends", None, False)
    out.append(Pair("bands tables<=48K", bt(12033), bt(12034), "palette", ("lds2<=cap",) + TWO_PASS_ONLY))
    return tuple(out)


MAGNITUDE_IN_PAIR = (20480, 20481)   # launch_magnitude_in: (M + 1) * 8 <= 160 KiB


@functools.lru_cache(maxsize=1)
def mixed_ends() -> tuple:
    """for every compile-time plan that a stream can run to pixels: (plan, mode, Pair or None, note) -- the largest row table that still fits
    and the first that does not, by f_max at 1024 rows or, where the whole axis fits, by the row count"""
    out = []
    for P in sorted(MIX_THREADS):
        for real in (False, True):
            W = P if real else P // 2
            if (not real and P % 2) or W in ls.SMOOTH_EXCLUDED or not (ls.smooth7(2 * W) and 2 * W <= ls.MIX_MAX_P):
                continue
            if not ls.mixed_is_fixed(P):
                continue
            cfg = Config(W=W, channels=1 if real else 2)
            target = "real column<=160K" if real else "mixed column<=image"
            fits = lambda c: mixed_predicates(c)[target]   # noqa: E731
            if not fits(_with(cfg, f_max=200.0, rows=1)):
                out.append((P, real, None, "no row table fits: the image has no room behind the column"))
                continue
            pair = None
            for base, knob, lo, hi in ((cfg, "f_max", 200.0, 1.0e5), (_with(cfg, f_max=1.0e5), "rows", 1024, 65536), (cfg, "rows", 1, 1024)):
                if fits(_with(base, **{knob: lo})) and not fits(_with(base, **{knob: hi})):
                    pair = _pair(target, base, knob, lo, hi, True, f"mixed-ends-{P}-{'real' if real else 'lr'}")
                    break
            assert pair is not None, (P, real)     # 65536 rows are 65536 samples at least: no image holds them
            out.append((P, real, pair, ""))
    return tuple(out)


def _class_reps() -> list:
    reps = {
        (256, 8, 12): Config(), (256, 8, 0): Config(rows=1025),
        (256, 10, 12): Config(W=2400, f_max=12000.0), (256, 10, 0): Config(W=2400, f_max=12000.0, rows=1025),
        (256, 16, 0): Config(W=3000, f_max=8000.0), (512, 8, 0): Config(W=4096), (512, 16, 0): Config(W=4800, f_max=16000.0),
        (1024, 8, 0): Config(W=8192), (1024, 10, 0): Config(W=9600, f_max=16000.0),
    }
    out = []
    for shape, cfg in reps.items():
        for pal in THREE_PALETTES:
            for ch in ((1, 2) if pal is SEQ256 else (2,)):
                c = _with(cfg, palette=pal, channels=ch, interp=(ch + shape[0] // 256) % 2)
                out.append(Context(f"class {shape} {pal.tag} ch {ch}", c, f"class-{shape[0]}-{shape[1]}-{shape[2]}", True if pal.n == 256 else None))
    for staged, W, narrow in ((True, 10240, False), (False, 20736, True)):
        for pal in THREE_PALETTES:
            c = _with(Config(W=W, f_max=24000.0, **(dict(rows=64) if narrow else {})), palette=pal, channels=2)
            out.append(Context(f"class column {'staged' if staged else 'global'} {pal.tag}", c, "class-column", True if pal.n == 256 else None, batch=staged))
    return out


def _extras() -> list:
    out = []
    add = lambda name, group, cfg, **kw: out.append(Context(name, cfg, group, **kw))   # noqa: E731
    for R in (1, 255, 256, 257, 1023, 1024, 1025):
        add(f"rows {R}", "rows", Config(rows=R, channels=1 + R % 2), proof=True)
    add("rows 65536", "rows-65536", Config(rows=65536, channels=2), proof=True)
    # few rows over a wide axis: rows of 255 and of 256 samples (bisected over f_max so that the top row has exactly that many)
    for want in (255, 256):
        f = bisect(Config(rows=4, f_min=200.0), "f_max", 400.0, 24000.0, lambda c: row_table(c).max_count <= want)[0]
        cfg = Config(rows=4, f_min=200.0, f_max=f)
        assert row_table(cfg).max_count == want, (want, row_table(cfg).max_count)
        add(f"a row of {want} samples", "row-counts", cfg, proof=True)
        add(f"a row of {want} samples, (l, r)", "row-counts", replace(cfg, channels=2, interp=1), proof=True)
    # axes that clamp: the top rows all at the last bin, the bottom rows all below one bin
    add("f_max far above Nyquist", "clamping", Config(f_max=400000.0, rows=512), proof=True)
    add("f_min below one bin", "clamping", Config(f_min=0.01, f_max=20000.0, channels=2), proof=True)
    add("both, cosine", "clamping", Config(f_min=0.5, f_max=96000.0, rows=300, interp=1), proof=True)
    add("both, W 4800", "clamping", Config(W=4800, f_min=0.5, f_max=96000.0, rows=300, channels=2), proof=True)
    # single_rows masks at W 2048 (wg4096's row pass) -- the axis chosen so that whole blocks of 256 rows hold one sample each
    # (0000 over three blocks: with four, a row of two samples in block 0 needs idx_255 ln(f_max / f_min) / R >= 2, and at M 2047 that
    # product is below 1 for every axis)
    add("single_rows 0000", "single-rows", Config(rows=520, f_min=2800.0, f_max=20500.0, channels=2), proof=True)
    add("single_rows 0011", "single-rows", Config(), proof=True)
    add("single_rows 1111", "single-rows", Config(f_min=32.0, f_max=700.0), proof=True)
    add("single_rows partial last block", "single-rows", Config(rows=600, f_min=32.0, f_max=900.0, channels=2), proof=True)
    add("sample rate 44100.9", "sample-rate", Config(sample_rate=44100.9), proof=True)
    add("sample rate 44100.9, W 2205", "sample-rate", Config(W=2205, sample_rate=44100.9, f_max=20000.0), proof=True)
    # palettes: sizes, both branches, both LUT index rules
    for n in (2, 7, 255, 256, 257, 4096, 40000, 65536):
        for stereo in (False, True):
            for mode in (0, 1):
                cfg = Config(palette=Palette("ramp", "ramp", n, stereo), lut_index_mode=mode, channels=2, interp=mode)
                add(f"palette {n}{' diverging' if stereo else ''} rule {mode}", f"palette-{n}", cfg, proof=True if n == 256 else None, batch=n in (7, 256))
    # the far tables beside a column that no LDS holds: render_far_tables_kernel<false>
    for stereo in (False, True):
        cfg = _with(Config(W=20736, rows=64, f_max=24000.0, palette=Palette("ramp", "ramp", 65536, stereo), channels=2, interp=int(stereo)))
        add(f"palette 65536{' diverging' if stereo else ''} W 20736", "palette-65536-long", cfg, batch=False)
    add("callback gradient", "palette-callback", Config(palette=Palette("scheme", "turbo", 0, False), channels=2))
    add("callback gradient, diverging", "palette-callback", Config(palette=Palette("scheme", "red_blue", 0, True), channels=2))
    # the two proofs, either way
    add("proof passes: default", "proofs", Config(), proof=True)
    add("proof passes: min_db -110", "proofs", Config(min_db=-110.0, max_db=-20.0), proof=True)
    add("proof passes: diverging alpha", "proofs", Config(palette=DIV256, channels=2), proof=True)
    add("proof fails: unreachable top levels", "proofs", Config(min_db=-70.0, max_db=400.0), proof=False)
    add("proof fails: unreachable top levels, diverging", "proofs", Config(min_db=-70.0, max_db=400.0, palette=DIV256, channels=2), proof=False)
    add("proof fails: narrow span", "proofs", Config(min_db=NARROW_DB[0], max_db=NARROW_DB[1]), proof=False)
    add("proof fails: narrow span, diverging", "proofs", Config(min_db=NARROW_DB[0], max_db=NARROW_DB[1], palette=DIV256, channels=2), proof=False)
    add("proof fails: narrow span, W 4800", "proofs", Config(W=4800, min_db=NARROW_DB[0], max_db=NARROW_DB[1], channels=2), proof=False)
    add("walk forced", "proofs", Config(flags=("lut_walk",)), proof=True)
    # launch_magnitude_in's own switch
    for W in MAGNITUDE_IN_PAIR:
        add(f"magnitude_in W {W}", "long-windows", _with(Config(rows=16, f_min=100.0, f_max=200.0, channels=2), W=W), proof=True, batch=False)
    return out


# a dB span so narrow that float32's dB ramp cannot follow the seed's line: near -40 dB a float32 moves in steps of 2^-18 dB, so this span
# holds about 131 float32 dB values for 256 levels (255 alpha bytes) -- levels are skipped.  tests/test_pixel_plans.py computes the margin
NARROW_DB = (-40.0, -39.9995)


@functools.lru_cache(maxsize=1)
def sweep() -> tuple:
    """every Context of the sweep, in a fixed order, names unique"""
    out = []
    for p in pairs():
        out += [p.a, p.b]
    for _, _, p, _ in mixed_ends():
        if p is not None:
            out += [p.a, p.b]
    out += _class_reps()
    out += _extras()
    seen, uniq = set(), []
    for c in out:
        assert c.name not in seen, c.name
        seen.add(c.name)
        uniq.append(c)
    return tuple(uniq)


def chunks() -> dict:
    """{case id of the GPU sweep: [Context, ...]}"""
    out = {}
    for c in sweep():
        out.setdefault(c.group, []).append(c)
    return out
