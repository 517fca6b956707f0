"""Guarded arenas for tests/test_gpu_bounds.py, and the sample and chunk arithmetic those tests are held to (a plain helper: no GPU, no
torch at import time; tests/test_bounds_arena.py checks it on hand-computed cases).

An arena is ONE device allocation viewed as int32 words, [front guard | payload | back guard].  An output arena's guards hold GUARD_WORD
and are compared as integers after the call; its payload is prefilled with a pattern no kernel result can leave behind unnoticed (+inf,
then all ones).  An input arena holds the stream as its payload and the quiet NaN in every word around it, so that a read outside the
stream (a record count one frame, one channel or one row too generous) poisons the result instead of returning the zero a torch
allocation usually holds there."""
from __future__ import annotations

from dataclasses import dataclass

GUARD_WORD = 0xA5A5A5A5      # both guards of an output arena
NAN_WORD = 0x7FC00000        # the quiet NaN around (and, where a test poisons it, inside) an input stream
INF_F32 = 0x7F800000         # output prefill, first pass: +inf survives a max, so a peak column that was loaded before its first store shows
INF_F16 = 0x7C00
BYTE_FILL = 0xA5
ALL_ONES = 0xFFFFFFFF        # output prefill, second pass: a NaN (f32 and f16), byte 0xFF
MIN_GUARD_BYTES = 64 << 10
WORKSPACE_BYTES = 192 << 20  # sgx_api.hip: the bounded workspace of the two-kernel routes


def as_i32(word: int) -> int:
    """a 32-bit pattern as the signed value an int32 tensor holds"""
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word & 0x80000000 else word


def prefill_word(kind: str, second_pass: bool) -> int:
    """the 32-bit word an output payload of element kind "f32", "f16" or "u8" is prefilled with"""
    if second_pass:
        return ALL_ONES
    return {"f32": INF_F32, "f16": INF_F16 | INF_F16 << 16, "u8": BYTE_FILL * 0x01010101}[kind]


def guard_bytes(row_bytes: int) -> int:
    """max(one output row, 64 KiB), rounded up to 8 bytes"""
    g = max(int(row_bytes), MIN_GUARD_BYTES)
    return (g + 7) // 8 * 8


@dataclass(frozen=True)
class Layout:
    payload_offset: int     # bytes from the allocation's start: [0, payload_offset) is the front guard
    payload_bytes: int
    back_offset: int        # = payload_offset + payload_bytes: [back_offset, total_bytes) is the back guard
    total_bytes: int

    @property
    def words(self):
        """(front, payload, back, total) in 32-bit words"""
        return self.payload_offset // 4, self.payload_bytes // 4, (self.total_bytes - self.back_offset) // 4, self.total_bytes // 4


def layout(payload_bytes: int, row_bytes: int, odd: bool, base_mod16: int = 0, mod4: bool = False) -> Layout:
    """[front guard | payload | back guard] for an allocation whose address is base_mod16 modulo 16 (a multiple of 8).  The payload
    starts on a multiple of 16 bytes, or in the odd variant at 8 modulo 16 -- the weakest alignment include/sgx.h promises to serve
    (the front guard grows by 8 bytes where that takes it).  mod4: 4 further bytes, the 4-but-not-8-byte aligned mono stream of
    edge_signals' align4 row.  Both guards are at least guard_bytes(row_bytes)."""
    assert payload_bytes % 4 == 0 and base_mod16 % 8 == 0 and 0 <= base_mod16 < 16
    g = guard_bytes(row_bytes)
    off = g
    if (base_mod16 + off) % 16 != (8 if odd else 0):
        off += 8
    if mod4:
        off += 4
    back = off + payload_bytes
    return Layout(off, payload_bytes, back, back + g)


def needed_samples(route, first: int, n: int):
    """[lo, hi): the samples frames [first, first + n) are a function of (include/sgx.h: frame t reads [t H, t H + W) alone).  On paired
    rows the frame range is first widened to whole pairs by global index: the partner frame shares the transform, and its rounding
    (tests/test_gpu_edges.py allows the same).  The caller clips hi to the stream's last whole frame: a partner the stream does not
    hold has no samples."""
    assert n >= 1 and first >= 0
    end = first + n
    if route.paired:
        first -= first % 2
        end += end % 2
    return first * route.H, (end - 1) * route.H + route.W


# ---- the chunk loops over the workspace (a restatement of sgx_api.hip, in the manner of edge_signals.large_chunk) ----------------
def mags_bytes_per_frame(W: int, pairs: int) -> int:
    return pairs * (W - 1) * 2 * 4


def render_chunk(W: int, pairs: int) -> int:
    """frames per chunk of sgx_render_batch on the two-kernel route: WORKSPACE_BYTES / the magnitudes of a frame, at least 1"""
    return max(WORKSPACE_BYTES // mags_bytes_per_frame(W, pairs), 1)


def bands_chunk(W: int, pairs: int) -> int:
    """frames per chunk of sgx_bands_batch on the two-kernel route: the same workspace, the same magnitudes"""
    return render_chunk(W, pairs)


def fbank_chunk(W: int, pairs: int) -> int:
    """frames per chunk of sgx_fbank_batch on the workspace route: the same workspace, the same magnitudes"""
    return render_chunk(W, pairs)


def fbank_cross_chunk(W: int, pairs: int) -> int:
    """frames per chunk of sgx_fbank_cross_batch on the workspace route: a frame's complex rows are two magnitude rows' bytes
    (in_workspace_chunks with rows_per_frame = 2), at least 1"""
    return max(WORKSPACE_BYTES // (2 * mags_bytes_per_frame(W, pairs)), 1)


# ---- the ranges of the Welch calls (a restatement of psd_reduce, sgx_api.hip, and of Geometry, sgx_psd.hpp) -------------------------
WELCH_BLOCK = 32                # include/sgx.h: frames per block of the float32 chain


def welch_row_bytes(W: int, pairs: int, cross: bool) -> int:
    """a row of the Welch calls and a block's partial row alike: the magnitudes of a frame (psd), twice that (csd)"""
    return mags_bytes_per_frame(W, pairs) * (2 if cross else 1)


def welch_cap(W: int, pairs: int, cross: bool) -> int:
    """rows (or partial rows) the workspace holds; 0 where one row is larger than all of it"""
    return WORKSPACE_BYTES // welch_row_bytes(W, pairs, cross)


@dataclass(frozen=True)
class WelchRange:
    blocks: tuple           # [b_lo, b_hi) of the call's blocks
    frames: tuple           # [f_lo, f_hi) of the call's frames
    pieces: tuple           # ((f, f + k, resume), ...): the rows launches of the range; resume: the block launch loads its partials
    reads_carry: bool       # the combine continues the column's float64 sums from the carry row
    writes_carry: bool      # ... and leaves them there: the column ends in a later range


@dataclass(frozen=True)
class WelchPlan:
    cap: int
    fpb: int                # frames per block, at most
    per: int                # blocks per range, at most
    piece: int              # frames per rows launch where a block's rows do not fit beside one partial row, else 0
    carried: bool           # a column has more blocks than a range: taken alone, its sums in the carry row between ranges
    row_slots: int          # rows in front of the partial rows (0: the stage calls, whose rows are the caller's)
    ranges: tuple

    @property
    def workspace_rows(self):
        """rows the workspace is grown to: the row slots and `per` partial rows behind them"""
        return self.row_slots + self.per

    @property
    def resumed(self):
        return any(p[2] for r in self.ranges for p in r.pieces)


def welch_ranges(W: int, pairs: int, cross: bool, n: int, group: int, own_rows: bool, cap: int = None) -> WelchPlan:
    """The ranges psd_reduce takes a call of n frames in columns of `group` in.  own_rows: the batch calls, whose rows go to the front
    of the workspace; else the stage calls.  cap: the rows the workspace holds, by default that of (W, pairs, cross)."""
    assert n >= 1 and group >= 1
    if cap is None:
        cap = welch_cap(W, pairs, cross)
    g = min(group, n)
    bpc = (g + WELCH_BLOCK - 1) // WELCH_BLOCK
    full, rem = divmod(n, g)
    every = full * bpc + (rem + WELCH_BLOCK - 1) // WELCH_BLOCK

    def column_end(j):
        return n if n - j * g < g else (j + 1) * g

    def block_first(b):
        return (b // bpc) * g + (b % bpc) * WELCH_BLOCK

    def block_end(b):
        f, ce = block_first(b), column_end(b // bpc)
        return ce if ce - f < WELCH_BLOCK else f + WELCH_BLOCK

    def column_block_end(j):
        return every if every - j * bpc < bpc else (j + 1) * bpc

    fpb = min(g, WELCH_BLOCK)
    per, piece = cap, 0
    if own_rows:
        if cap >= fpb + 1:
            per = cap // (fpb + 1)
        else:
            per, piece = 1, (cap - 1 if cap > 1 else 1)
    per = min(max(per, 1), every)
    carried = bpc > per
    if not carried:
        per -= per % bpc
    row_slots = min(piece if piece else per * fpb, n) if own_rows else 0
    ranges, b = [], 0
    while b < every:
        j = b // bpc
        m = min(every - b, per)
        if carried:
            m = min(m, column_block_end(j) - b)
        f_lo, f_hi = block_first(b), block_end(b + m - 1)
        pieces, f = [], f_lo
        while f < f_hi:
            k = min(f_hi - f, piece) if piece else f_hi - f
            pieces.append((f, f + k, f != f_lo))
            f += k
        reads = carried and b != j * bpc
        writes = carried and b + m != column_block_end(j)
        ranges.append(WelchRange((b, b + m), (f_lo, f_hi), tuple(pieces), reads, writes))
        b += m
    return WelchPlan(cap, fpb, per, piece, carried, row_slots, tuple(ranges))


WELCH_MAX = 2 ** 64 - 1         # group = SIZE_MAX: one column of all frames


def welch_first_carried(W: int, pairs: int, cross: bool) -> int:
    """the fewest frames whose one column (group = SIZE_MAX) a batch call carries: more blocks than a range holds"""
    cap = welch_cap(W, pairs, cross)
    per = cap // (WELCH_BLOCK + 1) if cap >= WELCH_BLOCK + 1 else 1
    return WELCH_BLOCK * per + 1


def welch_carried_route(routes, cross: bool = False):
    """(frames, route) of the route with the fewest frames whose group = SIZE_MAX column is carried, kernel 11 left out (its rows go
    through a scratch of their own: tests/test_gpu_psd.py carries a column there)"""
    served = [r for r in routes if r.kernel != 11 and not (cross and r.channels == 1)]
    return min(((welch_first_carried(r.W, r.pairs, cross), r) for r in served), key=lambda t: (t[0], t[1].W, t[1].channels, t[1].H))


def welch_odd_seam(W: int, pairs: int, groups=range(1, 65)):
    """(group, frames) of the first group whose batch call ends its first range on an odd frame, with the fewest frames that reach a
    second range of at least two frames; None where no group of `groups` has one"""
    cap = welch_cap(W, pairs, False)
    for g in groups:
        long = welch_ranges(W, pairs, False, cap + g + 3, g, True)  # (more frames than the workspace holds rows: at least two ranges)
        seam = long.ranges[0].frames[1]
        if len(long.ranges) >= 2 and seam % 2:
            frames = seam + 3
            assert welch_ranges(W, pairs, False, frames, g, True).ranges[0].frames[1] == seam
            return g, frames
    return None


N_BANK_FILTERS = 263            # fbank_reference.edge_bank: the bank of the bounds sweep
FUSED_BANK_KERNEL = 2           # info.stft_kernel of the 4096-point kernels, the only ones with a fused bank mode


def fbank_fused(route, cross: bool = False) -> int:
    """what sgx_fbank_fused / sgx_fbank_cross_fused must answer on a row of edge_signals.ROUTES for a bank within the fused size
    (include/sgx.h): the 4096-point kernels, not on frame pairs, not on the complex mono transform; the cross sums need an (l, r) pair"""
    fused = route.kernel == FUSED_BANK_KERNEL and not route.paired and "complex_mono" not in route.flags
    if cross:
        fused = fused and route.channels >= 2
    return 1 if fused else 0


PEAK_SUB_NUM, PEAK_SUB_DEN = 9, 64  # sgx_bands_peak_batch: kSubNum / kSubDen of a column per frame for the two-level reduction


def peak_per_frame(W: int, pairs: int, R: int, two_kernel: bool) -> int:
    """bytes of workspace per frame of a chunk on sgx_bands_peak_batch's workspace route: the band column, on the two-kernel bands
    route the magnitudes in front of it, and behind it 9 / 64 of a column (rounded up) for the sub-columns"""
    col_bytes = pairs * R * 2 * 4
    return col_bytes + (mags_bytes_per_frame(W, pairs) if two_kernel else 0) + (col_bytes * PEAK_SUB_NUM + PEAK_SUB_DEN - 1) // PEAK_SUB_DEN


def peak_chunk(W: int, pairs: int, R: int, n: int, group: int, two_kernel: bool = True) -> int:
    """frames per chunk of sgx_bands_peak_batch's workspace route for a call of n frames in columns of `group`:
    (WORKSPACE_BYTES - 2 columns) / per_frame, at most n, and, where a column fits, `chunk -= chunk % g` (whole columns per chunk)"""
    col_bytes = pairs * R * 2 * 4
    g = min(group, n)
    chunk = (WORKSPACE_BYTES - 2 * col_bytes) // peak_per_frame(W, pairs, R, two_kernel) if WORKSPACE_BYTES > 2 * col_bytes else 0
    chunk = min(max(chunk, 1), n)
    if g <= chunk:
        chunk -= chunk % g
    return chunk


def peak_chunks(W: int, pairs: int, R: int, n: int, group: int, two_kernel: bool = True) -> list:
    """[(done, m, column, accumulate)] of that loop: a chunk never runs past the end of the column it starts in when g > chunk
    (m trimmed to (j + 1) g - done), and accumulates into its column unless it starts on the column's first frame"""
    g = min(group, n)
    chunk = peak_chunk(W, pairs, R, n, group, two_kernel)
    out, done = [], 0
    while done < n:
        j = done // g
        m = min(n - done, chunk)
        if g > chunk:
            m = min(m, (j + 1) * g - done)
        out.append((done, m, j, done != j * g))
        done += m
    return out


# ---- the runs of the fused peak-hold route (a restatement of peak_align_run, stft4096_wg.hpp, and of the job split of the launchers) ----
def peak_align_run(per: int, frames_per_job: int, group: int) -> int:
    """jobs per workgroup, rounded up to whole columns of `group` frames where that lengthens the run by at most 1 / 32"""
    unit = group if group % frames_per_job == 0 else group * frames_per_job
    run = per * frames_per_job
    if unit > run // 32:
        return per
    return (run + unit - 1) // unit * unit // frames_per_job


def fused_peak_run(n: int, group: int, n_cu: int, frames_per_job: int = 2) -> int:
    """frames per persistent workgroup of sgx_bands_peak_batch's fused route for a call of n frames: four workgroups per CU, each a
    contiguous run of jobs of `frames_per_job` frames (2: the real-input 4096-point kernel of a mono stream; 1: the (l, r) kernel).
    Workgroup b accumulates frames [b run, (b + 1) run); a column that crosses such an end is finished by the combine pass."""
    jobs = (n + frames_per_job - 1) // frames_per_job
    blocks = n_cu * 4
    per = max((jobs + blocks - 1) // blocks, 1)
    return peak_align_run(per, frames_per_job, min(group, n)) * frames_per_job
