"""The case table of tests/stream_cases.py (what tests/test_gpu_stream_routes.py runs on a held stream) checked on the CPU: every row of
edge_signals.ROUTES is in it, with every entry point the row's route serves, no case twice; every helper pass a launcher could put on the
wrong stream is taken by some case; the stand-alone cases name every kernel body of the pixel stage."""
import collections

import bounds_arena as ba
import edge_signals as es
import far_offsets as fo
import stream_cases as sc
from spectrogram_rs_amd import _lib


def test_every_row_of_routes_is_in_the_table():
    rows = sc.by_row()
    assert list(rows) == [r.name for r in es.ROUTES]
    assert len(rows) == len(es.ROUTES) >= 45


def test_every_entry_point_the_route_serves_is_listed():
    rows = sc.by_row()
    always = (set(sc.BATCH) | set(sc.STAGE)) - {"fbank_cross", "csd_3"}
    assert {"fbank", "fbank_mags", "fbank_cross_spec", "psd_3", "psd_mags", "csd_spec"} <= always
    for r in es.ROUTES:
        listed = set(rows[r.name])
        assert always <= listed, (r.name, always - listed)
        # the cross sums from PCM: every context with an (l, r) pair (the stage serves the mono rows as well)
        assert ("fbank_cross" in listed) == (r.channels >= 2), r.name
        # the Welch cross means from PCM likewise (sgx_csd_spec serves the mono rows)
        assert ("csd_3" in listed) == (r.channels >= 2), r.name
        assert sc.psd_fused(r) == 0
        # the inverse: every length an in-LDS kernel serves, i.e. every row but kernel 11's
        assert ("istft" in listed) == (r.kernel != 11), r.name
        assert listed == set(sc.entries_served(r))
    assert sum(1 for r in es.ROUTES if r.kernel == 11) == 8
    # every entry is a symbol of the C ABI, and no batch or stage entry point of the ABI that takes a context and enqueues is left out
    exported = {name for name, _, _ in _lib.SIGNATURES}
    assert set(sc.SYMBOL.values()) <= exported and len(set(sc.SYMBOL.values())) == len(sc.ENTRIES) == len(sc.SYMBOL)
    enqueue_only = {n for n in exported if n.startswith(("sgx_stft_batch", "sgx_render_", "sgx_bands_", "sgx_istft_batch"))}
    enqueue_only -= {"sgx_bands_fused", "sgx_bands_peak_fused"}
    banks = {n for n in exported if n.startswith("sgx_fbank_")} - {"sgx_fbank_create", "sgx_fbank_destroy", "sgx_fbank_filters", "sgx_fbank_fused",
                                                                      "sgx_fbank_cross_fused"}
    assert banks == {"sgx_fbank_batch", "sgx_fbank_mags", "sgx_fbank_cross_batch", "sgx_fbank_cross_spec"}
    welch = {n for n in exported if n.startswith(("sgx_psd_", "sgx_csd_"))} - {"sgx_psd_fused", "sgx_csd_fused"}
    assert welch == {"sgx_psd_batch", "sgx_csd_batch", "sgx_psd_mags", "sgx_csd_spec"}
    assert enqueue_only | banks | welch | {"sgx_magnitude_in", "sgx_checksum_add"} == set(sc.SYMBOL.values())
    assert sc.READS["psd_mags"] == "stft" and sc.READS["csd_spec"] == "complex"
    assert set(sc.READS) == {"istft"} | set(sc.STAGE) and set(sc.READS.values()) <= set(sc.BATCH)
    assert sc.HOST_WAITS == {}


def test_no_case_is_listed_twice():
    count = collections.Counter((c.row, c.entry) for c in sc.CASES)
    assert max(count.values()) == 1
    assert len(sc.CASES) == (len(es.ROUTES) * (len(sc.ENTRIES) - 3) + sum(1 for r in es.ROUTES if r.kernel != 11)
                             + 2 * sum(1 for r in es.ROUTES if r.channels >= 2))
    for cases in (sc.VIEW_CASES, sc.IMAGE_CASES, sc.PIXEL_CASES, sc.WELCH_CASES):
        names = [c.name for c in cases]
        assert len(names) == len(set(names))
    assert len({n for n, _, _ in sc.REBIND_CASES}) == len(sc.REBIND_CASES)


def test_the_streams_are_ragged_and_short():
    for r in es.ROUTES:
        F = sc.frames_of(r)
        assert F % sc.PEAK_GROUP != 0 and F > sc.PEAK_GROUP, r.name          # a ragged last column
        pcm_bytes = ((F - 1) * r.H + r.W) * r.channels * 4
        complex_bytes = F * r.pairs * (r.W - 1) * 16
        assert pcm_bytes <= 64 << 20 and complex_bytes <= 128 << 20, (r.name, pcm_bytes, complex_bytes)
    assert sc.SEED_A != sc.SEED_B


def test_every_helper_pass_is_taken_by_some_case():
    # with the routes the contexts report at the default 1024 rows and the viridis table: fused pixels and bands on the 4096-point kernels,
    # neither on W 8192, kernel 11, the ladders and the generic kernel
    taken = collections.defaultdict(set)
    for r in es.ROUTES:
        fused = r.kernel == 2
        for e in sc.entries_served(r):
            for h in sc.helpers(r, e, fused, fused):
                taken[h].add((r.name, e))
    assert set(taken) == set(sc.HELPERS)
    assert {row for row, _ in taken["deinterleave"]} == {"k1_ch4", "k1_ch8"}
    assert {e for _, e in taken["deinterleave"]} == set(sc.BATCH)
    assert {row for row, _ in taken["k16_plane"]} == {"k16_mono_h512"}
    assert {e for _, e in taken["to_half"]} == {"f16"}
    assert {es.ROUTE[row].kernel for row, _ in taken["to_half"]} == {0, 4, 10, 11}
    assert {e for _, e in taken["workspace_magnitude_in"]} == {"bands", "peak_3"}
    assert {e for _, e in taken["peak_combine"]} == {"peak_3"}
    assert {row for row, _ in taken["peak_combine"]} == {r.name for r in es.ROUTES if r.kernel == 2 and not r.paired}
    assert {es.ROUTE[row].kernel for row, _ in taken["large_passes"]} == {11} and {e for _, e in taken["large_passes"]} == set(sc.BATCH)
    assert {es.ROUTE[row].kernel for row, _ in taken["ladder"]} == {4}
    assert len(taken["inverse"]) == len(es.ROUTES) - 8
    # the bank calls: one kernel on the 4096-point kernels (behind the de-interleave pass on 4 and 8 channels, above), the workspace and
    # the stage everywhere else -- the frame pairs and the complex mono transform of that kernel included
    assert {e for _, e in taken["workspace_fbank"]} == {"fbank"} and {e for _, e in taken["workspace_fbank_cross"]} == {"fbank_cross"}
    unfused = {r.name for r in es.ROUTES if r.kernel != 2} | {"k1_complex_mono", "k1_paired_mono"}
    assert {row for row, _ in taken["workspace_fbank"]} == unfused
    assert {row for row, _ in taken["workspace_fbank_cross"]} == {n for n in unfused if es.ROUTE[n].channels >= 2}
    for row in ("k1_ch4", "k1_ch8"):
        assert sc.helpers(es.ROUTE[row], "fbank", True, True) == sc.helpers(es.ROUTE[row], "fbank_cross", True, True) == {"deinterleave"}
    assert sc.helpers(es.ROUTE["k1_lr_h256"], "fbank_cross", True, True) == set()
    assert sc.helpers(es.ROUTE["k16_mono_h512"], "fbank", False, False) == {"k16_plane", "workspace", "workspace_fbank"}
    assert sc.helpers(es.ROUTE["bluestein_w23"], "fbank_cross", False, False) == {"ladder", "workspace", "workspace_fbank_cross"}
    assert sc.helpers(es.ROUTE["k1r_h256"], "fbank_mags", True, True) == set()
    # the Welch calls: never fused -- the rows into the workspace behind the rows' own helpers on EVERY row, the 4096-point kernels
    # included, then block partials and the combine; the stages are those two kernels alone
    welch = {"workspace_psd_blocks", "workspace_psd_combine"}
    for h in welch:
        assert {e for _, e in taken[h]} == {"psd_3", "csd_3", "psd_mags", "csd_spec"}
        assert {row for row, e in taken[h] if e == "psd_3"} == {r.name for r in es.ROUTES}
        assert {row for row, e in taken[h] if e == "csd_3"} == {r.name for r in es.ROUTES if r.channels >= 2}
    for r in es.ROUTES:
        for fused in (False, True):
            assert sc.helpers(r, "psd_3", fused, fused) == sc.rows_helpers(r) | {"workspace"} | welch, r.name
            assert sc.helpers(r, "psd_mags", fused, fused) == sc.helpers(r, "csd_spec", fused, fused) == welch, r.name
    assert sc.helpers(es.ROUTE["k1_ch8"], "csd_3", True, True) == {"deinterleave", "workspace"} | welch
    assert sc.helpers(es.ROUTE["k16_mono_h512"], "psd_3", False, False) == {"k16_plane", "workspace"} | welch
    assert sc.helpers(es.ROUTE["bluestein_w23"], "csd_3", False, False) == {"ladder", "workspace"} | welch
    assert sc.helpers(es.ROUTE["large_w6001_chunks"], "psd_3", False, False) == {"large_passes", "workspace"} | welch
    # one run of a persistent workgroup of the fused peak kernel is one frame here (23 frames on 4 n_cu workgroups): every column of three
    # frames crosses runs, so the combine pass writes every column
    assert sc.FRAMES < 4 * 64


def test_the_families_are_the_routes_own():
    fam = {r.name: sc.family(r) for r in es.ROUTES}
    assert fam["k48_lr"] == fam["k48_paired_mono"] == "w4800" and fam["mixed_w2400_real"] == fam["mixed_w2400_ch4"] == "mixed"
    assert fam["bluestein_w1102"] == fam["bluestein_w23"] == "bluestein" and fam["chirpz_w1102_lr"] == "chirpz"
    assert collections.Counter(fam.values()) == {"wg4096": 9, "w16384": 5, "w4800": 2, "mixed": 10, "chirpz": 3, "bluestein": 2,
                                                 "generic": 6, "large": 8}
    # the same families far_offsets names one row each of
    assert {sc.family(fo.family_route(f)) for f in fo.FAMILIES} == set(fam.values())


def test_the_welch_case_is_carried_and_pieced():
    assert [c.cross for c in sc.WELCH_CASES] == [False, True]
    for c in sc.WELCH_CASES:
        assert (c.W, c.channels, c.frames, c.group) == (32768, 64, 36, ba.WELCH_MAX)      # tests/test_gpu_psd.py's context
        plan = ba.welch_ranges(c.W, c.channels // 2, c.cross, c.frames, c.group, True)
        assert plan.carried and plan.piece and plan.resumed
        assert [(r.reads_carry, r.writes_carry) for r in plan.ranges] == [(False, True), (True, False)]
        assert sum(len(r.pieces) for r in plan.ranges) >= 3                              # rows launches, each with kernel 11's passes


def test_the_stand_alone_cases_cover_the_pixel_stage():
    bodies = {c.body for c in sc.PIXEL_CASES}
    assert bodies == {c.body for c in fo.PIXEL_CASES if c.entry != "render_bands"}
    assert {"magnitude_in_kernel<true>", "magnitude_in_kernel<false>", "render_far_tables_kernel<true>"} <= bodies
    assert any(c.n_lut == 40706 for c in sc.PIXEL_CASES)
    for c in sc.PIXEL_CASES:   # the same contexts as the far-offset cases, a handful of columns
        far = next(f for f in fo.PIXEL_CASES if f.name == c.name)
        assert (c.body, c.entry, c.W, c.R, c.large, c.n_lut, c.n_ranges) == (far.body, far.entry, far.W, far.R, far.large, far.n_lut, far.n_ranges)
        assert 1 < c.cols <= 16
    # the copy wraps (two pieces and three), and every second write ends where the ring began
    assert len(sc.VIEW_CASES) == 2 and all(v.viewport < v.frames and 2 * v.frames % v.viewport == 0 and v.frames % v.viewport for v in sc.VIEW_CASES)
    assert sorted(-(-v.frames // v.viewport) for v in sc.VIEW_CASES) == [2, 3]
    # the ring laps itself and ends at an offset other than 0: the scrolled read composes two parts
    assert all(i.W != 2048 and i.width < sc.FRAMES and sc.FRAMES % i.width for i in sc.IMAGE_CASES)
    assert [kw["window_samples"] for _, kw, _ in sc.REBIND_CASES] == [8192] * 4
    assert [m for _, _, m in sc.REBIND_CASES if m.startswith("fbank_")] == ["fbank_batch"]
