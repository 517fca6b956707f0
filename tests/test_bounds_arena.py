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
