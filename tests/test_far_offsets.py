"""tests/far_offsets.py without a GPU: every placed frame or row straddles its mark, the pieces tile their call, the replay keeps alignment
and parity, the tables reach every row and family, nothing breaks the cap -- and a truncated frame offset is seen."""
import numpy as np
import pytest

import bounds_arena as ba
import edge_signals as es
import far_offsets as fo
import pixel_plans as pp

INPUT = fo.input_cases() + fo.index_cases()
HOPS = fo.hop_cases()
OUTPUTS = fo.output_cases()


def test_arenas_and_marks():
    assert fo.arena_bytes("A") == (1 << 32) + (64 << 20) and fo.arena_bytes("B") == (1 << 34) + (64 << 20)
    assert [(a, m * 4) for a, _, m in fo.INPUT_MARKS] == [("A", 1 << 31), ("A", 1 << 32), ("B", 1 << 33), ("B", 1 << 34)]
    for arena, _, mark in fo.INPUT_MARKS:
        assert mark < fo.ARENA_FLOATS[arena]
    assert fo.arena_bytes("B") / 2 ** 30 == pytest.approx(16.0625)


@pytest.mark.parametrize("case", INPUT, ids=lambda c: c.id)
def test_input_case_straddles_its_mark(case):
    r = case.route
    lo, hi = fo.window(r, case.f0 + 2)
    assert lo <= case.mark < hi, "the mark lies outside frame f0 + 2"
    assert case.f0 >= 1, "no frame before the first one for a paired row's partner"
    seen = set()
    for first, n, n_samples in case.calls():
        assert n == fo.FRAMES_PER_CALL and first < case.f0 + 2 < first + n - 1, "the frames before and after it belong to the call"
        assert n_samples <= fo.stream_samples(r, case.arena)
        a, b = fo.owned(r, first, n, n_samples)
        assert 0 <= a < b <= n_samples and (b + fo.base_offset(r)) * r.channels <= fo.ARENA_FLOATS[case.arena]
        assert a * r.channels <= case.mark < b * r.channels
        assert (n_samples - r.W) // r.H + 1 >= first + n, "the stream holds fewer frames than the call asks for"
        seen.add(first % 2)
    assert seen == {0, 1}, "both parities"
    if case.part == 3:
        assert r.H == 1 and case.arena == "B" and (case.f0 + 2) * r.channels == case.mark and case.f0 + 2 in (1 << 31, 1 << 32)


def test_owned_samples_of_a_paired_row():
    r = es.ROUTE["k1_paired_mono"]
    # frames 3 .. 7 of a stream that ends with frame 7: pairs (2, 3) .. (6, 7), nothing beyond
    assert fo.owned(r, 3, 5, 7 * 256 + 2048) == (2 * 256, 7 * 256 + 2048)
    # frames 4 .. 8: frame 9 is the partner of 8 -- where the stream holds it
    assert fo.owned(r, 4, 5, 8 * 256 + 2048) == (4 * 256, 8 * 256 + 2048)
    assert fo.owned(r, 4, 5, 1 << 30) == (4 * 256, 9 * 256 + 2048)
    assert fo.owned_windows(r, 4, 5, 1 << 30) == [(t * 256, t * 256 + 2048) for t in range(4, 10)]
    assert fo.owned(es.ROUTE["k1r_h256"], 3, 5, 1 << 30) == (3 * 256, 7 * 256 + 2048)


@pytest.mark.parametrize("case", INPUT, ids=lambda c: c.id)
def test_replay_keeps_alignment_and_parity(case):
    r = case.route
    for first, n, n_samples in case.calls():
        lo, hi = fo.owned(r, first, n, n_samples)
        rp = fo.replay_of(r, first, lo, hi)
        assert rp.first == first % 2 and rp.shift % (2 * r.H) == 0 and rp.shift // r.H + rp.first == first
        assert 0 <= rp.lo < rp.hi == rp.n_samples and rp.hi - rp.lo == hi - lo
        assert rp.n_samples <= (fo.FRAMES_PER_CALL + 2) * r.H + r.W, "the replay is not compact"
        # the replay holds the call's frames, and as many whole frames as the call saw where the stream ended with them
        assert (rp.n_samples - r.W) // r.H + 1 >= rp.first + n
        for base in (0x7F0000000000, 0x7F0000000008):
            src = base + (fo.base_offset(r) + rp.shift * r.channels) * 4
            for dst in (0x7E0000000000, 0x7E0000000004, 0x7E0000000008, 0x7E000000000C):
                pad = fo.replay_pad(src, dst)
                assert 0 <= pad < 4 and (dst + pad * 4) % 16 == src % 16


@pytest.mark.parametrize("case", HOPS, ids=lambda c: c.id)
def test_hop_case(case):
    r, small = case.route, case.small
    step = r.H * r.channels * 4
    e = int(case.what[-2:])
    assert (step < 1 << e) == case.what.startswith("below") and abs(step - (1 << e)) <= 8
    assert (r.W, r.channels, r.flags, r.kernel) == (small.W, small.channels, small.flags, small.kernel) and small.H < small.W
    frames = set()
    for first, n, n_samples in case.calls():
        assert n_samples <= fo.stream_samples(r, case.arena)
        assert (n_samples - r.W) // r.H + 1 >= first + n
        for a, b in fo.owned_windows(r, first, n, n_samples):
            assert b - a == r.W and b * r.channels <= fo.ARENA_FLOATS[case.arena]
            frames.add(a // r.H)
    assert frames >= ({0, 1} if case.arena == "A" else {0, 1, 2})
    assert [c[0] for c in case.calls()] == ([0] if case.arena == "A" else [0, 1])


@pytest.mark.parametrize("case", OUTPUTS, ids=lambda c: c.id)
def test_output_case(case):
    rb = case.row_bytes
    assert rb % 4 == 0 and case.route.pairs == 1
    assert case.output_bytes >= (1 << 32) + 2 * rb > case.output_bytes - rb
    assert case.input_bytes + case.output_bytes <= fo.CASE_CAP_BYTES
    probes = case.probes()
    for m in fo.OUTPUT_MARKS:
        k = m // rb
        assert k * rb <= m < (k + 1) * rb and {k - 1, k, k + 1} <= set(probes) and 0 < k - 1 and k + 1 <= case.rows - 1
    assert probes[0] == 0 and probes[-1] == case.rows - 1
    # the pieces tile the call exactly, each below 2^31 bytes
    at = 0
    for a, n in case.pieces():
        assert a == at and n >= 1 and n * rb < fo.PIECE_LIMIT
        at += n
    assert at == case.rows and len(case.pieces()) >= 3
    assert case.frames == case.rows * (2 if case.kind == "peak_2" else 1)
    assert case.R in (fo.ROWS_DEFAULT, fo.ROWS_MAX) and (case.R == fo.ROWS_DEFAULT or case.route.kernel == 11)


def test_tables_reach_every_row_and_family():
    assert {c.row for c in fo.input_cases()} == {r.name for r in es.ROUTES}
    assert len(fo.input_cases()) == len(es.ROUTES) * len(fo.INPUT_MARKS)
    named = ["k1r", "k1_lr", "k1_paired", "k48_lr", "k48_paired", "mixed_fixed", "mixed_real", "mixed_runtime", "mixed_runtime_real",
             "chirpz", "bluestein", "generic", "k16_lr", "k16_mono", "k16_paired", "large_direct", "large_chirp"]
    assert list(fo.FAMILIES) == named
    assert {c.family for c in HOPS} == set(named) and len(HOPS) == len(named) * 4 * 2
    assert {c.family for c in OUTPUTS} == set(named) - {"mixed_runtime_real"}
    # every family through every kind but the filterbank calls; those on the fused family and on one workspace family with a short hop
    # ... and the Welch calls at group 1 on the two 4096-point families: the mono rows (the weighted deal of their launches) and (l, r)
    assert fo.OUTPUT_KINDS[-4:-2] == list(fo.BANK_KINDS) == ["fbank", "fbank_cross"]
    assert fo.OUTPUT_KINDS[-2:] == list(fo.WELCH_KINDS) == ["psd_1", "csd_1"]
    assert {(c.family, c.kind) for c in OUTPUTS} == ({(f, k) for f in fo.OUTPUT_FAMILIES for k in fo.OUTPUT_KINDS[:-4]}
                                                     | {(f, k) for f in ("k1_lr", "k48_lr") for k in fo.BANK_KINDS}
                                                     | {("k1r", "psd_1"), ("k1_lr", "csd_1")})
    welch = {(c.family, c.kind): c for c in OUTPUTS if c.kind in fo.WELCH_KINDS}
    assert {k: (c.row_bytes, c.rows, c.group, c.R) for k, c in welch.items()} == {
        ("k1r", "psd_1"): (2047 * 8, 262275, 1, 1024),           # 2^32 / 16376 = 262 272.5 rows, and two
        ("k1_lr", "csd_1"): (2047 * 16, 131139, 1, 1024)}        # 2^32 / 32752 = 131 136.3 rows, and two
    for (family, kind), c in welch.items():
        # hundreds of ranges at the mono rows, the frame passed to the rows launches up to the call's last
        plan = ba.welch_ranges(c.route.W, 1, kind == "csd_1", c.frames, 1, True)
        assert len(plan.ranges) == {"psd_1": 43, "csd_1": 43}[kind] and not plan.carried and not plan.piece
        assert plan.ranges[-1].frames[1] == c.frames and plan.ranges[1].frames[0] == {"psd_1": 6147, "csd_1": 3073}[kind]
        assert fo.family_route(family).kernel == 2 and fo.family_route(family).channels == (1 if kind == "psd_1" else 2)
    banks = {(c.family, c.kind): c for c in OUTPUTS if c.kind in fo.BANK_KINDS}
    assert {k: (c.row_bytes, c.rows) for k, c in banks.items()} == {
        ("k1_lr", "fbank"): (8192, 524290), ("k48_lr", "fbank"): (8192, 524290),                   # 2^32 / 8 KiB = 524288 rows, and two
        ("k1_lr", "fbank_cross"): (16384, 262146), ("k48_lr", "fbank_cross"): (16384, 262146)}     # 2^32 / 16 KiB = 262144 rows, and two
    assert all(c.input_bytes + c.output_bytes <= fo.CASE_CAP_BYTES and c.R == fo.ROWS_DEFAULT for c in banks.values())
    assert fo.family_route("k1_lr").kernel == 2 and fo.family_route("k48_lr").kernel == 9 and fo.family_route("k48_lr").H == 93
    # the family rows are what their names say (edge_signals' route bits)
    R4, R8 = es.R4, es.R8
    fam = fo.family_route
    assert fam("k1r").bits_set & R8 and fam("k1_lr").kernel == 2 and fam("k1_paired").paired and fam("k48_paired").paired
    assert fam("k48_lr").kernel == 9 and fam("k16_paired").paired and fam("k16_paired").kernel == fam("k16_mono").kernel == 10
    assert fam("mixed_fixed").bits_set & R4 and fam("mixed_real").bits_set & R8 and fam("mixed_runtime").bits_clear & R4
    assert fam("mixed_runtime_real").bits_clear & R4 and fam("mixed_runtime_real").bits_set & R8
    assert fam("chirpz").kernel == 4 and fam("chirpz").bits_set & R4 and fam("bluestein").kernel == 4 and fam("bluestein").bits_clear & R4
    assert fam("generic").kernel == 0 and fam("large_direct").kernel == fam("large_chirp").kernel == 11
    assert not es.large_plan(fam("large_direct").W)[3] and es.large_plan(fam("large_chirp").W)[3]
    # part 3: every family's kernel, as a mono or an (l, r) context
    rows = fo.INDEX_MONO_ROWS + fo.INDEX_LR_ROWS
    assert all(fo.route(n).channels == 1 for n in fo.INDEX_MONO_ROWS) and all(fo.route(n).channels == 2 for n in fo.INDEX_LR_ROWS)
    for f in named:
        r = fam(f)
        assert any((fo.route(n).kernel, fo.route(n).bits_set, fo.route(n).paired) == (r.kernel, r.bits_set, r.paired) for n in rows) \
            or any((fo.route(n).W, fo.route(n).flags) == (r.W, r.flags) for n in rows), f
    assert len(fo.index_cases()) == 2 * len(fo.INDEX_MONO_ROWS) + len(fo.INDEX_LR_ROWS)


# ---- the method detects what it is for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in INPUT if c.row in ("k1_lr_h256", "generic_w64_mono", "large_w1m_lr", "k1r_h256")],
                         ids=lambda c: c.id)
def test_a_truncated_frame_offset_reads_nan(case):
    """(first_frame + j) * H * C in 64 bits reads the frame's own samples.  Truncated at the width of the case's mark (a uint32 float
    offset at 2^32 floats, a uint32 byte offset at 2^30 floats, one that lost its sign bit at 2^29) it reads, for every frame that
    starts beyond the mark, a lower address of the same arena: NaN, in every sample"""
    r = case.route
    C, W = r.channels, r.W
    bits = case.mark.bit_length() - 1
    assert case.mark == 1 << bits
    for first, n, n_samples in case.calls():
        lo, hi = fo.owned(r, first, n, n_samples)
        own = [(lo * C, hi * C)]
        beyond = 0
        for j in range(n):
            off = fo.frame_offset(first, j, r.H, C)
            assert off == fo.window(r, first + j)[0]
            assert not np.isnan(fo.read_model(own, off, W * C)).any()
            wrapped = fo.frame_offset(first, j, r.H, C, bits=bits)
            if off >= case.mark:
                assert wrapped == off - case.mark < lo * C
                assert np.isnan(fo.read_model(own, wrapped, W * C)).all(), "a wrapped offset must land on NaN"
                beyond += 1
            else:
                assert wrapped == off
        assert beyond >= 1, "no frame of the call starts beyond the mark: the comparison would pass a truncated offset"


def test_a_truncated_frame_index_reads_nan():
    case = next(c for c in fo.index_cases() if c.row == "k1r_h256" and c.what == "frame 2^32")
    r = case.route
    first, n, n_samples = case.calls()[0]
    lo, hi = fo.owned(r, first, n, n_samples)
    for j in range(n):
        wrapped = (first + j) & 0xFFFFFFFF
        assert not np.isnan(fo.read_model([(lo, hi)], (first + j) * r.H, r.W)).any()
        assert (wrapped != first + j) == (j >= 2)
        if j >= 2:   # frames 2^32 .. 2^32 + 2 become frames 0 .. 2: the head of the arena
            assert np.isnan(fo.read_model([(lo, hi)], wrapped * r.H, r.W)).all()


def test_a_truncated_row_offset_leaves_prefill():
    """an output row offset truncated to uint32 writes the rows beyond 2^32 bytes over the first rows: the rows beyond keep the prefill
    (check a), the first rows hold other frames (checks b and c)"""
    case = fo.output_case("k1r", "stft")
    written = np.zeros(case.rows, bool)
    for k in range(case.rows):
        off = (k * case.row_bytes) & 0xFFFFFFFF
        if off % case.row_bytes == 0:
            written[off // case.row_bytes] = True
    assert not written[(1 << 32) // case.row_bytes + 1:].any()
    assert ba.prefill_word("f32", False) == ba.INF_F32


def test_inverse_cases():
    for which, name in fo.INVERSE_ROWS.items():
        r = fo.route(name)
        assert r.channels == 2 and r.kernel != 11 and es._smooth7(2 * r.W) == (which == "route_1")
        far = fo.inverse_route(which, fo.INVERSE_FAR_H)
        assert far.H > far.W and 2 * far.H > 1 << 31 and 4 * far.H > 1 << 32 and fo.INVERSE_FAR_FRAMES == 6
        out = fo.inverse_route(which, fo.INVERSE_OUT_H)
        H, W, F = out.H, out.W, fo.inverse_out_frames()
        N = (F - 1) * H + W
        assert H > W + 2 * fo.INVERSE_MARGIN and N * 8 > (1 << 32) + 8 * H and N > 1 << 29
        probes = fo.inverse_probe_frames(F)
        for sample in (1 << 28, 1 << 29):   # byte 2^31 and byte 2^32 of the (l, r) output lie inside a frame, its neighbours are probed
            t = sample // H
            assert t * H + fo.INVERSE_MARGIN <= sample < t * H + W - fo.INVERSE_MARGIN and {t - 1, t, t + 1} <= set(probes) and t + 1 < F
        at = 0
        for a, n in fo.sample_pieces(N, 2):
            assert a == at and n * 8 < fo.PIECE_LIMIT
            at += n
        assert at == N and len(fo.sample_pieces(N, 2)) >= 3
        assert N * 8 + F * (W - 1) * 16 <= fo.CASE_CAP_BYTES


@pytest.mark.parametrize("case", fo.PIXEL_CASES, ids=lambda c: c.id)
def test_pixel_case(case):
    n_in, n_out = case.cols * case.in_col_bytes, case.cols * case.out_col_bytes
    assert n_in > (1 << 32) + case.in_col_bytes and n_out > (1 << 32) + case.out_col_bytes, "both buffers pass 2^32 bytes, a column beyond"
    if case.entry != "render_bands":
        assert 0.9 <= case.in_col_bytes / case.out_col_bytes <= 1.1, "input and output do not cross together"
        assert n_in + n_out <= fo.CASE_CAP_BYTES
    else:
        # bands in are 8 bytes a row, pixels out 4: no row count brings an output past 2^32 bytes under 12 GiB = 3 * 2^32 with its input.
        # The case is the least there is: the fewest columns whose output passes the mark by two columns, nothing more
        assert case.in_col_bytes == 2 * case.out_col_bytes and case.cols == fo.rows_for(case.out_col_bytes)
        assert n_in + n_out == 3 * n_out < 3 * ((1 << 32) + 3 * case.out_col_bytes)
    probes = set(case.probes())
    for m in fo.OUTPUT_MARKS:
        for cb in (case.in_col_bytes, case.out_col_bytes):
            k = m // cb
            assert k * cb <= m < (k + 1) * cb and {k - 1, k} <= probes and (k + 1 in probes or k + 1 >= case.cols)
    at = 0
    for a, n in case.pieces():
        assert a == at and n * case.in_col_bytes < fo.PIECE_LIMIT and n * case.out_col_bytes < fo.PIECE_LIMIT
        at += n
    assert at == case.cols
    # the body the case names is the one the launchers' inequalities give on gfx950's 160 KiB, for this context's row table (the GPU test
    # evaluates the same function on what the device and the context report)
    cfg = pp.Config(W=case.W, rows=case.R, channels=2, palette=pp.Palette("ramp", "ramp", case.n_lut), flags=("large_transforms",) * case.large)
    assert case.large == pp.needs_large(case.W) and case.R <= fo.ROWS_MAX and 2 <= case.n_lut <= 65536
    assert fo.pixel_body(case.entry, case.M, pp.row_table(cfg).n_samples, case.n_lut, fo.LDS_CAP) == case.body
    assert fo.LDS_CAP == pp.LDS_CAP


@pytest.mark.parametrize("case", fo.BANK_STAGE_CASES, ids=lambda c: c.id)
def test_bank_stage_case(case):
    """sgx_fbank_mags / sgx_fbank_cross_spec: the column index times n_filters (the stage kernels' `col * p.n_filters`) passes 2^31 and 2^32
    bytes of output; the columns are as short as a context takes, so the case is its output and a sixteenth of it"""
    assert case.n_filters == fo.BANK_FILTERS == 1024 and case.W == 64
    assert (case.in_col_bytes, case.out_col_bytes) == {"fbank_mags": (63 * 8, 8192), "fbank_cross_spec": (63 * 16, 16384)}[case.entry]
    n_in, n_out = case.cols * case.in_col_bytes, case.cols * case.out_col_bytes
    assert (1 << 32) + 2 * case.out_col_bytes <= n_out < (1 << 32) + 3 * case.out_col_bytes
    assert n_in + n_out <= fo.CASE_CAP_BYTES and n_in < fo.PIECE_LIMIT
    probes = set(case.probes())
    for m in fo.OUTPUT_MARKS:
        k = m // case.out_col_bytes
        assert k * case.out_col_bytes <= m < (k + 1) * case.out_col_bytes and {k - 1, k, k + 1} <= probes and k + 1 <= case.cols - 1
        # the element index the kernel forms, col * n_filters float2s (float4s), passes 2^28 and 2^29 there: bytes 2^31 and 2^32
        assert k * case.n_filters * (case.out_col_bytes // case.n_filters) == m
    assert {0, case.cols - 1} <= probes
    at = 0
    for a, n in case.pieces():
        assert a == at and n >= 1 and n * case.out_col_bytes < fo.PIECE_LIMIT
        at += n
    assert at == case.cols and len(case.pieces()) >= 3
    first, count, weights = fo.far_bank(case.W - 1)
    assert len(first) == 1024 and (count == 1).all() and first[0] == 0 and first[1] == case.W - 2 and int(first.max()) < case.W - 1
    assert weights.dtype == np.float32 and (np.abs(weights) >= 2.0 ** -6).all() and (np.abs(weights) <= 1.0).all() and (weights < 0).any()
    for M in (2047, 2399):                                   # the banks of the batch cases: within the fused size, bins all over the column
        f, c, w = fo.far_bank(M)                             # (bin M - 1, put in by hand, may repeat one of the scattered ones)
        assert len(set(f.tolist())) >= 1023 and int(f.max()) == M - 1 and int(c.sum()) == 1024 <= 16384


@pytest.mark.parametrize("case", fo.WELCH_STAGE_CASES, ids=lambda c: c.id)
def test_welch_stage_case(case):
    """sgx_psd_mags / sgx_csd_spec: the frame index times the row's elements (the block kernel's `f * elems + e`) and the column index times
    them (the combine's `j * elems + e`) pass bytes 2^31 and 2^32; the rows are as short as a context takes"""
    assert case.W == 64 and case.groups == (1, 2)
    rb = case.row_bytes
    assert rb == {"psd_mags": 63 * 8, "csd_spec": 63 * 16}[case.entry]
    F = case.frames
    assert (1 << 32) + 2 * rb <= F * rb < (1 << 32) + 3 * rb
    assert 2 * F * rb <= fo.CASE_CAP_BYTES
    for group in case.groups:
        cols = case.cols(group)
        marks_in, marks_out = case.crossed(group)
        assert marks_in == fo.OUTPUT_MARKS and marks_out == (fo.OUTPUT_MARKS if group == 1 else fo.OUTPUT_MARKS[:1])
        probes = set(case.probes(group))
        assert {0, cols - 1} <= probes and max(probes) == cols - 1 and min(probes) == 0
        for m in marks_out:
            k = m // rb
            assert k * rb <= m < (k + 1) * rb and {k - 1, k, k + 1} <= probes and k + 1 <= cols - 1
        for m in marks_in:       # the column whose frames hold the mark of the input
            f = m // rb
            assert f * rb <= m < (f + 1) * rb and f + 1 <= F - 1 and {f // group - 1, f // group, f // group + 1} & probes >= {f // group - 1, f // group}
        if group == 2:           # frame 2 j + 1 of the column at the output's mark 2^31 lies past the input's 2^32
            k = marks_out[0] // rb
            assert (2 * k + 1) * rb > 1 << 32 and F % 2 == 1                       # and the last column is one frame
        at = 0
        for a, n in case.pieces(group):
            assert a == at and n >= 1 and n * group * rb < fo.PIECE_LIMIT
            at += n
        assert at == cols and len(case.pieces(group)) >= 3


def test_pixel_cases_reach_every_body():
    assert [c.body for c in fo.PIXEL_CASES] == [
        "render_two_pass_kernel", "render_kernel<true>", "render_kernel<false>", "render_far_tables_kernel<true>", "magnitude_in_kernel<true>",
        "magnitude_in_kernel<false>", "render_bands_kernel"]
    # pixel_body against the restatement tests/pixel_plans.py keeps of launch_render and launch_magnitude_in
    for case in fo.PIXEL_CASES:
        cfg = pp.Config(W=case.W, rows=case.R, channels=2, palette=pp.Palette("ramp", "ramp", case.n_lut))
        n = pp.row_table(cfg).n_samples
        if case.entry == "magnitude_in":
            assert case.body == f"magnitude_in_kernel<{str(pp.magnitude_in_staged(cfg)).lower()}>"
        elif case.entry == "render_mags":
            for seeded in ((False, True) if case.n_lut == 256 else (False,)):
                cls = pp.render_class(cfg, seeded)
                want = "render_two_pass_kernel" if cls[0] == "two_pass" else \
                    f"{'render_kernel' if cls[2] else 'render_far_tables_kernel'}<{str(cls[1]).lower()}>"
                assert fo.pixel_body(case.entry, case.M, n, case.n_lut, fo.LDS_CAP) == want == case.body
