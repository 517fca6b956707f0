"""tests/bounds_arena.py on hand-computed cases: the arena layout, the samples a frame range owns, the chunk sizes (no GPU)."""
import pytest

import bounds_arena as ba
import edge_signals as es


def test_words_and_prefill():
    assert ba.as_i32(ba.GUARD_WORD) == -1515870811 and ba.as_i32(ba.NAN_WORD) == 2143289344 and ba.as_i32(ba.ALL_ONES) == -1
    assert ba.prefill_word("f32", False) == 0x7F800000
    assert ba.prefill_word("f16", False) == 0x7C007C00
    assert ba.prefill_word("u8", False) == 0xA5A5A5A5
    assert {ba.prefill_word(k, True) for k in ("f32", "f16", "u8")} == {0xFFFFFFFF}


@pytest.mark.parametrize("row_bytes,want", [
    (8, 65536),                 # a short row: 64 KiB
    (65536, 65536),
    (65537, 65544),             # rounded up to 8 bytes
    (70001, 70008),
    (((1 << 20) - 1) * 8, 8388600),   # a W 2^20 row of (l, r) magnitudes
])
def test_guard_bytes(row_bytes, want):
    assert ba.guard_bytes(row_bytes) == want


@pytest.mark.parametrize("args,offset,total", [
    ((400, 8, False, 0), 65536, 65536 + 400 + 65536),
    ((400, 8, True, 0), 65544, 65544 + 400 + 65536),        # the odd variant: 8 modulo 16
    ((400, 8, False, 8), 65544, 65544 + 400 + 65536),       # an allocation that itself sits at 8 modulo 16
    ((400, 8, True, 8), 65536, 65536 + 400 + 65536),
    ((4, 70001, True, 0), 70008, 70008 + 4 + 70008),        # 70008 = 8 modulo 16 already
    ((4, 70001, False, 0), 70016, 70016 + 4 + 70008),
])
def test_layout(args, offset, total):
    lay = ba.layout(*args)
    assert (lay.payload_offset, lay.total_bytes) == (offset, total)
    assert lay.back_offset == offset + args[0]
    assert (args[3] + lay.payload_offset) % 16 == (8 if args[2] else 0)
    front, payload, back, words = lay.words
    assert front + payload + back == words and front * 4 >= ba.guard_bytes(args[1]) and back * 4 == ba.guard_bytes(args[1])


def test_layout_of_the_align4_stream():
    lay = ba.layout(400, 8, False, 0, mod4=True)
    assert lay.payload_offset == 65540 and lay.payload_offset % 8 == 4


@pytest.mark.parametrize("name,first,n,want", [
    ("k1_lr_h256", 0, 1, (0, 2048)),
    ("k1_lr_h256", 2, 3, (512, 3072)),                 # frames 2, 3, 4: [2 * 256, 4 * 256 + 2048)
    ("k48_lr", 3, 1, (279, 2679)),                     # first odd, unpaired: frame 3 alone, [3 * 93, 3 * 93 + 2400)
    ("large_w16384_lr", 1, 2, (8195, 32774)),          # H > W: [8195, 2 * 8195 + 16384), the gap between the frames included
    ("k1_paired_mono", 0, 2, (0, 2304)),               # a whole pair: nothing widened
    ("k1_paired_mono", 1, 1, (0, 2304)),               # first odd: frame 0 shares frame 1's transform
    ("k1_paired_mono", 1, 2, (0, 2816)),               # frames 1, 2 -> pairs (0, 1), (2, 3): [0, 3 * 256 + 2048)
    ("k1_paired_mono", 2, 3, (512, 3328)),             # frames 2, 3, 4 -> frame 5 joins: [512, 5 * 256 + 2048)
    ("k48_paired_mono", 3, 1, (186, 2679)),            # frame 3 -> pair (2, 3): [2 * 93, 3 * 93 + 2400)
    ("k1_complex_mono", 1, 1, (256, 2304)),            # mono, but every frame its own transform
])
def test_needed_samples(name, first, n, want):
    assert ba.needed_samples(es.ROUTE[name], first, n) == want


def test_chunk_sizes_w8192_r1024():
    # W 8192, (l, r), 1024 rows: a frame of magnitudes is 8191 * 8 = 65528 bytes, 3072 of them are 201 302 016 <= 192 MiB = 201 326 592
    # and 3073 are not
    assert ba.WORKSPACE_BYTES == 201326592
    assert ba.mags_bytes_per_frame(8192, 1) == 65528
    assert ba.render_chunk(8192, 1) == 3072 and ba.bands_chunk(8192, 1) == 3072
    # the peak route: column 8192 B + magnitudes 65528 B + ceil(8192 * 9 / 64) = 1152 B = 74872 B per frame;
    # (201326592 - 16384) / 74872 = 2688.7
    assert ba.peak_per_frame(8192, 1, 1024, True) == 74872
    assert ba.peak_chunk(8192, 1, 1024, 6000, 6000) == 2688
    assert ba.peak_chunk(8192, 1, 1024, 6000, 2689) == 2688      # g > chunk: the chunk stays
    assert ba.peak_chunk(8192, 1, 1024, 6000, 2688) == 2688
    assert ba.peak_chunk(8192, 1, 1024, 6000, 2687) == 2687      # chunk -= chunk % g
    assert ba.peak_chunk(8192, 1, 1024, 6000, 5) == 2685
    assert ba.peak_chunk(8192, 1, 1024, 100, 7) == 98            # at most n, then whole columns
    # on a fused bands route no magnitudes: 8192 + 1152 = 9344 B per frame, 201310208 / 9344 = 21544.3
    assert ba.peak_per_frame(2048, 1, 1024, False) == 9344
    assert ba.peak_chunk(2048, 1, 1024, 10 ** 6, 10 ** 6, two_kernel=False) == 21544


def test_fbank_chunk_sizes():
    # W 8192, (l, r): the magnitude rows of 3072 frames fill the workspace (above); a frame's complex rows are 2 * 65528 = 131056 bytes,
    # 1536 of them are 201 302 016 <= 201 326 592 and 1537 are not
    assert ba.fbank_chunk(8192, 1) == 3072 and ba.fbank_cross_chunk(8192, 1) == 1536
    # W 2400, (l, r): 2399 * 8 = 19192 bytes; 201326592 / 19192 = 10490.1, / 38384 = 5245.06
    assert ba.fbank_chunk(2400, 1) == 10490 and ba.fbank_cross_chunk(2400, 1) == 5245
    # W 2^20, (l, r): 8388600 bytes a frame: 24 frames of magnitudes (201326400), 12 of complex rows, one bin short of 25 and of 13
    assert ba.fbank_chunk(1 << 20, 1) == 24 and ba.fbank_cross_chunk(1 << 20, 1) == 12
    # four pairs at W 8192: 262112 bytes; 768.09 -> 768, 384.04 -> 384
    assert ba.fbank_chunk(8192, 4) == 768 and ba.fbank_cross_chunk(8192, 4) == 384
    # a frame larger than the workspace: one frame per chunk
    assert ba.fbank_cross_chunk(1 << 20, 16) == 1 and 2 * ba.mags_bytes_per_frame(1 << 20, 16) > ba.WORKSPACE_BYTES


def test_fbank_fused_rule():
    fused = {r.name: (ba.fbank_fused(r), ba.fbank_fused(r, cross=True)) for r in es.ROUTES}
    assert {n for n, v in fused.items() if v[0]} == {"k1r_h256", "k1r_h100", "k1r_h256_align4", "k1_lr_h256", "k1_lr_h58", "k1_ch4", "k1_ch8"}
    assert {n for n, v in fused.items() if v[1]} == {"k1_lr_h256", "k1_lr_h58", "k1_ch4", "k1_ch8"}
    assert fused["k1_complex_mono"] == (0, 0) and fused["k1_paired_mono"] == (0, 0) and fused["generic_w2048_lr"] == (0, 0)


def test_peak_chunk_loop():
    # one column over three chunks
    assert ba.peak_chunks(8192, 1, 1024, 6000, 6000) == [(0, 2688, 0, False), (2688, 2688, 0, True), (5376, 624, 0, True)]
    assert ba.peak_chunks(8192, 1, 1024, 6000, 6005) == ba.peak_chunks(8192, 1, 1024, 6000, 6000)
    # two columns, the second chunk trimmed to (j + 1) g - done = 4000 - 2688
    assert ba.peak_chunks(8192, 1, 1024, 6000, 4000) == [(0, 2688, 0, False), (2688, 1312, 0, True), (4000, 2000, 1, False)]
    # chunk + 1: one frame of every column in a chunk of its own
    assert ba.peak_chunks(8192, 1, 1024, 6000, 2689) == [(0, 2688, 0, False), (2688, 1, 0, True), (2689, 2688, 1, False),
                                                         (5377, 1, 1, True), (5378, 622, 2, False)]
    assert ba.peak_chunks(8192, 1, 1024, 6000, 2688) == [(0, 2688, 0, False), (2688, 2688, 1, False), (5376, 624, 2, False)]
    assert ba.peak_chunks(8192, 1, 1024, 6000, 2687) == [(0, 2687, 0, False), (2687, 2687, 1, False), (5374, 626, 2, False)]


@pytest.mark.parametrize("n,group,n_cu,fpj,want", [
    (5000, 5000, 256, 2, 6),         # 2500 jobs over 1024 workgroups: 3 jobs = 6 frames
    (4997, 7, 256, 2, 6),            # 2499 jobs: still 3; a unit of 14 frames is not within 6 / 32
    (5000, 7, 256, 1, 5),            # one frame per job: 5000 / 1024 -> 5
    (1000000, 8, 256, 2, 984),       # 489 jobs = 978 frames; whole columns of 8 within 978 / 32 = 30: 984
    (1000000, 7, 256, 2, 980),       # an odd group: units of 14 frames, 70 of them
    (1000000, 977, 256, 2, 978),     # 1954 > 30: the run stays
    (10, 3, 256, 2, 2),              # fewer jobs than workgroups: one job each
])
def test_fused_peak_run(n, group, n_cu, fpj, want):
    assert ba.fused_peak_run(n, group, n_cu, fpj) == want


# ---- the ranges of the Welch calls (bounds_arena.welch_ranges: a restatement of psd_reduce) ---------------------------------------------
def test_welch_row_counts_of_test_gpu_psd():
    # the rows tests/test_gpu_psd.py counts on: 8 channels at W 2048: 4 * 2047 * 8 = 65504 bytes, 201326592 / 65504 = 3073.5
    assert ba.welch_cap(2048, 4, False) == 3073
    # 8 channels at W 19200: 4 * 19199 * 8 = 614368 bytes: 327.7 rows, 163.8 complex rows
    assert (ba.welch_cap(19200, 4, False), ba.welch_cap(19200, 4, True)) == (327, 163)
    # 64 channels at W 32768: 32 * 32767 * 8 = 8388352 bytes, 64 bytes short of 8 MiB: 24 rows and 12 complex rows (not 22 and 11: what
    # the test needs of them, fewer than a block of 32 rows and its partial, holds of both)
    assert (ba.welch_cap(32768, 32, False), ba.welch_cap(32768, 32, True)) == (24, 12)
    # a row larger than the workspace: no row fits
    assert ba.welch_cap(2048, 16384, False) == 0 and ba.welch_row_bytes(2048, 16384, False) > ba.WORKSPACE_BYTES


def test_welch_plan_by_hand():
    # W 2048 with 8 channels at group 3: blocks of 3 frames, 3073 // 4 = 768 blocks a range, 2304 rows in front of 768 partial rows
    p = ba.welch_ranges(2048, 4, False, 2400, 3, True)
    assert (p.cap, p.fpb, p.per, p.piece, p.carried, p.row_slots, p.workspace_rows) == (3073, 3, 768, 0, False, 2304, 3072)
    assert [(r.blocks, r.frames) for r in p.ranges] == [((0, 768), (0, 2304)), ((768, 800), (2304, 2400))]
    assert all(r.pieces == ((r.frames[0], r.frames[1], False),) and not r.reads_carry and not r.writes_carry for r in p.ranges)
    # group 1: 3073 // 2 = 1536 frames a range
    assert [r.frames for r in ba.welch_ranges(2048, 4, False, 2400, 1, True).ranges] == [(0, 1536), (1536, 2400)]
    # the stage over the caller's rows: no row slots, the whole workspace partial rows
    q = ba.welch_ranges(2048, 4, False, 2400, 3, False)
    assert (q.row_slots, q.per, len(q.ranges)) == (0, 800, 1)
    # W 19200 with 8 channels, 400 frames: 327 // 33 = 9 blocks a range.  group 33 (2 blocks a column): 8 blocks = 4 columns a range;
    # one column of 400 frames has 13 blocks: carried over two ranges
    p = ba.welch_ranges(19200, 4, False, 400, 33, True)
    assert (p.per, p.carried, p.row_slots) == (8, False, 256) and [r.frames for r in p.ranges] == [(0, 132), (132, 264), (264, 396), (396, 400)]
    p = ba.welch_ranges(19200, 4, False, 400, ba.WELCH_MAX, True)
    assert (p.per, p.carried) == (9, True)
    assert [(r.frames, r.reads_carry, r.writes_carry) for r in p.ranges] == [((0, 288), False, True), ((288, 400), True, False)]
    # W 32768 with 64 channels, 36 frames: 24 rows: 23 frames a piece beside one partial row
    p = ba.welch_ranges(32768, 32, False, 36, 33, True)
    assert (p.cap, p.per, p.piece, p.carried, p.row_slots, p.workspace_rows) == (24, 1, 23, True, 23, 24)
    assert [(r.frames, r.pieces, r.reads_carry, r.writes_carry) for r in p.ranges] == [
        ((0, 32), ((0, 23, False), (23, 32, True)), False, True), ((32, 33), ((32, 33, False),), True, False),
        ((33, 36), ((33, 36, False),), False, False)]
    # no row fits: a frame a piece, two rows of workspace all the same
    p = ba.welch_ranges(2048, 16384, False, 3, 2, True)
    assert (p.cap, p.per, p.piece, p.row_slots, p.workspace_rows) == (0, 1, 1, 1, 2)
    assert [r.pieces for r in p.ranges] == [((0, 1, False), (1, 2, True)), ((2, 3, False),)]


@pytest.mark.parametrize("cap", [0, 1, 2, 3, 5, 32, 33, 34, 66, 67, 100, 1000])
@pytest.mark.parametrize("own_rows", [True, False])
def test_welch_ranges_partition_the_call(cap, own_rows):
    """the blocks of all ranges partition Geometry.blocks() and their frames [0, n); the pieces partition a range's frames and fit the row
    slots; the partial rows lie behind the row slots; the carry row is written before it is read, by the same column; and the whole is
    psd_reference.plan's (written from the same source at another time)"""
    import psd_reference as ref
    for n in (1, 2, 31, 32, 33, 64, 65, 100, 333):
        for group in (1, 2, 5, 31, 32, 33, 64, 65, 70, n, n + 10, ba.WELCH_MAX):
            p = ba.welch_ranges(64, 1, False, n, group, own_rows, cap=cap)
            geo = ref.Geometry(n, group)
            what = (cap, own_rows, n, group)
            assert p.ranges[0].blocks[0] == 0 and p.ranges[-1].blocks[1] == geo.blocks(), what
            assert p.ranges[0].frames[0] == 0 and p.ranges[-1].frames[1] == n, what
            holds_carry = False
            for a, b in zip(p.ranges, p.ranges[1:] + (None,)):
                assert a.blocks[0] < a.blocks[1] <= a.blocks[0] + p.per and a.frames[0] < a.frames[1], what
                if b is not None:
                    assert a.blocks[1] == b.blocks[0] and a.frames[1] == b.frames[0], what
                assert a.frames == (geo.block_first(a.blocks[0]), geo.block_end(a.blocks[1] - 1)), what
                assert a.pieces[0][0] == a.frames[0] and a.pieces[-1][1] == a.frames[1], what
                assert all(x[1] == y[0] for x, y in zip(a.pieces, a.pieces[1:])), what
                assert [x[2] for x in a.pieces] == [False] + [True] * (len(a.pieces) - 1), what
                if own_rows:
                    assert all(x[1] - x[0] <= p.row_slots for x in a.pieces), (what, "a rows launch writes into the partial rows")
                else:
                    assert len(a.pieces) == 1, what
                j0, j1 = a.blocks[0] // geo.bpc, (a.blocks[1] - 1) // geo.bpc
                if p.carried:
                    assert j0 == j1, (what, "a carried range holds blocks of two columns")
                    assert a.reads_carry == (a.blocks[0] != j0 * geo.bpc) and a.writes_carry == (a.blocks[1] != geo.column_block_end(j0)), what
                else:
                    assert a.blocks[0] == j0 * geo.bpc and a.blocks[1] == geo.column_block_end(j1), (what, "a range ends inside a column")
                    assert not a.reads_carry and not a.writes_carry, what
                assert a.reads_carry == holds_carry, (what, "the carry row is read before it was written, or left unread")
                holds_carry = a.writes_carry
            assert not holds_carry, what
            if own_rows:
                assert p.workspace_rows <= max(cap, 2), (what, "more workspace than the bound")
            other, (slots, per, carried) = ref.plan(n, group, cap, own_rows)
            assert (slots, per, carried) == (p.row_slots, p.per, p.carried), what
            assert other == [(r.blocks[0], r.blocks[1] - r.blocks[0], [(f, e - f, res) for f, e, res in r.pieces]) for r in p.ranges], what


def test_welch_cases_of_the_gpu_tests():
    """every case the GPU tests name shows the property it is there for"""
    import channel_counts as cc
    # tests/test_gpu_bounds.py, part E: a carried column on a family that is not kernel 11 -- the fewest frames of the route table
    for cross, frames in ((False, 737), (True, 353)):
        n, r = ba.welch_carried_route(es.ROUTES, cross)
        assert (n, r.name) == (frames, "k16_ch8_h300")
        p = ba.welch_ranges(r.W, r.pairs, cross, n, ba.WELCH_MAX, True)
        assert p.carried and len(p.ranges) == 2 and p.ranges[0].writes_carry and p.ranges[1].reads_carry and not p.piece
        assert not ba.welch_ranges(r.W, r.pairs, cross, n - 1, ba.WELCH_MAX, True).carried
    # ... and a seam of two ranges at an odd frame of a paired mono W 2048 context: group 1, 12294 // 2 = 6147 frames a range
    assert ba.welch_odd_seam(2048, 1) == (1, 6150)
    p = ba.welch_ranges(2048, 1, False, 6150, 1, True)
    assert [r.frames for r in p.ranges] == [(0, 6147), (6147, 6150)] and not p.carried
    # tests/test_gpu_bounds.py, part C: no group is carried on the two chunk rows at their 300 and 70 frames (a carried column needs
    # more blocks than a range holds: 32 * (cap // 33) + 1 frames and more)
    for name, frames in (("large_w6001_chunks", 300), ("large_w16384_ch4_chunks", 70)):
        r = es.ROUTE[name]
        assert max(9, r.min_frames) == frames
        for cross in (False, True):
            assert ba.welch_first_carried(r.W, r.pairs, cross) > frames
            for g in list(range(1, frames + 6)) + [ba.WELCH_MAX]:
                assert not ba.welch_ranges(r.W, r.pairs, cross, frames, g, True).carried, (name, cross, g)
    # tests/test_gpu_stream_routes.py: W 32768 with 64 channels, 36 frames, one column: carried and pieced, the second piece resumed
    for cross in (False, True):
        p = ba.welch_ranges(32768, 32, cross, 36, ba.WELCH_MAX, True)
        assert p.carried and p.piece and p.resumed and len(p.ranges) == 2
        assert p.ranges[0].writes_carry and p.ranges[1].reads_carry and len(p.ranges[0].pieces) >= 2
    # tests/test_gpu_psd.py: at least two ranges of whole columns at W 2048 with 8 channels
    p = ba.welch_ranges(2048, 4, False, 2400, 3, True)
    assert len(p.ranges) >= 2 and not p.carried and all(r.frames[0] % 3 == 0 for r in p.ranges)
    # tests/test_gpu_channel_counts.py: the rows of 32 768 channels: none, or fewer than a block and its partial
    caps = {c.name: (ba.welch_cap(c.W, c.pairs, False), ba.welch_cap(c.W, c.pairs, True)) for c in cc.CAP_ROWS}
    assert caps == {"generic_w64_cap": (24, 12), "bluestein_w23_cap": (69, 34), "mixed_w735_runtime_cap": (2, 1), "k1_h256_cap": (0, 0),
                    "k16_h512_cap": (0, 0)}
    for c in cc.CAP_ROWS:
        for cross in (False, True):
            p = ba.welch_ranges(c.W, c.pairs, cross, c.frames, ba.WELCH_MAX, True)
            assert (p.piece == 1) == (p.cap <= 2) and p.workspace_rows <= max(p.cap, 2)
