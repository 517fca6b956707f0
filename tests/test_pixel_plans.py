"""The pixel-plan sweep of tests/pixel_plans.py (what tests/test_gpu_pixel_plans.py runs on the GPU) checked on the CPU: that it is
deterministic, that its row tables are the oracle's, that every launch_render class the rules make reachable appears under a sequential and
a diverging 256-entry palette and under a palette of another size, that every inequality of the rules has its pair of contexts -- the
nearest reachable values on either side, differing in that inequality alone -- or its proof that it cannot bind, and that the named extras
are what their names say.  The sweep ended up with 205 contexts."""
import os
import re

import numpy as np

import length_sweep as ls
import oracle
import pixel_plans as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
N_CONTEXTS = 205


def test_the_sweep_is_deterministic():
    first = [(c.name, c.cfg, c.group, c.proof) for c in pp.sweep()]
    for f in (pp.sweep, pp.pairs, pp.mixed_ends, pp._row_table):
        f.cache_clear()
    again = [(c.name, c.cfg, c.group, c.proof) for c in pp.sweep()]
    assert first == again and len(first) == len({n for n, *_ in first}) == N_CONTEXTS
    assert sum(len(v) for v in pp.chunks().values()) == N_CONTEXTS
    # the end the issue names: the default axis crosses the fused limit between these two doubles (2301 and 2303 padded slots)
    p = [p for p in pp.pairs() if p.target == "wg slots<=2302"][0]
    assert (p.a.cfg.f_max, p.b.cfg.f_max) == (22432.486030686257, 22432.48603068626)
    assert (pp.row_table(p.a.cfg).padded, pp.row_table(p.b.cfg).padded) == (2301, 2303)
    assert (pp.row_table(pp.Config()).n_samples, pp.row_table(pp.Config()).padded) == (2173, 2264)


def test_row_tables_are_the_oracles():
    seen = set()
    for c in pp.sweep():
        g = c.cfg
        key = (g.W, g.sr_u32, g.rows, g.f_min, g.f_max)
        if key in seen:
            continue
        seen.add(key)
        t = pp.row_table(g)
        rows = range(g.rows) if g.rows <= 2048 else list(range(0, g.rows, 37)) + [g.rows - 1]
        for py in rows:
            f0, f1 = np.float32(oracle.log_unmap(g.f_min, g.f_max, py, 0, g.rows)), np.float32(oracle.log_unmap(g.f_min, g.f_max, py + 1, 0, g.rows))
            assert t.counts[py] == oracle.num_samples_in(g.M, g.sr_u32, float(f0), float(f1)), (c.name, py)
        counts = np.array(t.counts)
        assert t.n_samples == counts.sum() and t.padded == t.n_samples + sum(1 for n in t.counts if n >= 4 and n % 2 == 0)
        assert t.max_count == counts.max() and t.max_first == t.n_samples - t.counts[-1]
        assert t.n_samples <= g.rows + max(g.M - 1, 0)          # what the proofs of deadness lean on
    assert np.array_equal(oracle.bin_edges(7, 100.0, 8000.0), np.array([oracle.log_unmap(100.0, 8000.0, p, 0, 7) for p in range(8)]).astype(np.float32))


def test_the_constants_and_thread_tables_are_the_sources():
    threads = {row[0]: row[-1] for row in ls.macro("MIX_FIXED_PLANS") + ls.macro("MIX_FIXED4_PLANS")}
    assert threads == pp.MIX_THREADS and set(threads) == set(ls.MIX_FIXED)
    assert {row[0]: row[-1] for row in ls.macro("MIX_REAL_RENDER_PLANS")} == pp.MIX_REAL_THREADS
    assert tuple(row[0] for row in ls.macro("MIX_REAL2_RENDER_PLANS")) == pp.MIX_REAL2
    assert tuple(row[0] for row in ls.macro("MIX_FIXED4_PLANS")) == pp.MIX_FOUR_STAGE
    kern = open(os.path.join(CSRC, "sgx_kernels.hip")).read()
    for text in ("c->M <= 1024 * 10 && lds2 <= lds_cap", "n_samples <= 256 * 12 && c->R <= 1024 && n_samples < 65536", "(size_t)160 * 1024",
                 "fit >= 4 ? 256u : (fit >= 2 ? 512u : 1024u)", "(c->M + nt - 1) / nt > 16", "256 * sizeof(uint2)", "lds <= 48 * 1024",
                 "if (need <= 8) e2 = in_regs", "else if (need <= 10) e2 = in_regs"):
        assert text in kern, text
    hpp = open(os.path.join(CSRC, "stft4096_wg.hpp")).read()
    ks1 = int(re.search(r"constexpr int kS1 = (\d+);", hpp).group(1))
    assert "kBufComplex = 16 * kS1" in hpp and "kColSlots = 2050" in hpp and 16 * ks1 - 2050 == pp.WG_MAX_SLOTS
    assert "constexpr int kTCells = 512;" in open(os.path.join(CSRC, "sgx_internal.hpp")).read()
    wg = open(os.path.join(CSRC, "stft4096_wg.hip")).read()
    assert "c->tab.rows.size() <= 1024" in wg and "r.count >= 4 && (r.count & 1u) == 0" in wg
    assert "if (r.count >= 65536u || samples.size() >= 65536) fusable = false;" in wg       # the row word's 16 bits of count: pp.wg_predicates


def test_every_reachable_class_appears_under_three_palettes():
    by_class = {}
    for c in pp.sweep():
        p = c.cfg.palette
        if c.cls is None:                    # a callback gradient: only the library counts its colour steps
            assert p.kind == "scheme"
            continue
        kind = "other" if p.n != 256 else ("div256" if p.stereo else "seq256")
        by_class.setdefault(c.cls, set()).add(kind)
    for cls in pp.ALL_CLASSES:
        assert by_class.get(cls, set()) >= {"seq256", "div256", "other"}, (cls, by_class.get(cls))
    # render_class can return nothing else but the two far-table forms of the per-column kernel, which only palettes beyond 40 705 entries
    # reach: the column staged (W 2048) and read where it lies (W 20481, W 20736), sequential and diverging
    assert set(by_class) - set(pp.ALL_CLASSES) == set(pp.FAR_CLASSES)
    for cls in pp.FAR_CLASSES:
        far = [c for c in pp.sweep() if c.cls == cls]
        assert {c.cfg.palette.stereo for c in far} == {False, True} and all(c.cfg.palette.n > 40705 for c in far), cls
    # both colour rules, both interpolators and both channel counts occur in every two-pass shape
    for shape in pp.TWO_PASS_SHAPES:
        ctx = [c for c in pp.sweep() if c.cls == ("two_pass",) + shape]
        assert {c.cfg.interp for c in ctx} == {0, 1} and {c.cfg.channels for c in ctx} == {1, 2}, shape
        assert {c.seeded for c in ctx} == {True, False}, shape


def _all_pairs():
    return list(pp.pairs()) + [p for _, _, p, _ in pp.mixed_ends() if p is not None]


def test_every_inequality_has_its_pair_or_its_proof():
    names = set()
    for c in pp.sweep():
        names |= set(pp.all_predicates(c.cfg, c.seeded))
    names.discard("nt")
    covered = {p.target for p in _all_pairs()}
    assert covered | set(pp.DEAD) == names and not covered & set(pp.DEAD), (names - covered - set(pp.DEAD), covered & set(pp.DEAD))
    # both tails of the LDS inequalities, both modes of the mixed-radix plans
    for target in ("lds2<=cap", "fit>=2", "fit>=4", "R<=1024"):
        assert {p.a.seeded for p in pp.pairs() if p.target == target} == {True, False}, target
    nt_of = lambda p: {pp.predicates(p.a.cfg, True).get("nt"), pp.predicates(p.b.cfg, True).get("nt")}   # noqa: E731
    assert [sorted(nt_of(p)) for p in pp.pairs() if p.target == "need<=8"] == [[256], [512], [1024]]
    assert [sorted(nt_of(p)) for p in pp.pairs() if p.target == "grow"] == [[256, 512], [512, 1024]]
    # ... and both members read the last bins, which a prefetch of too few bins per thread leaves out: the axis ends at Nyquist
    for p in pp.pairs():
        if p.target in ("need<=8", "need<=10", "grow", "M<=10240"):
            for c in (p.a.cfg, p.b.cfg):
                top = oracle.index_of(float(oracle.bin_edges(c.rows, c.f_min, c.f_max)[-1]), c.M, c.sr_u32)
                assert top == c.M - 1, (p.a.name, top)
    ends = {(P, real): pair for P, real, pair, _ in pp.mixed_ends()}
    fused_real = sorted(P for P in pp.MIX_THREADS if P in ls.ALL_SMOOTH_W and P not in ls.SMOOTH_EXCLUDED and ls.mixed_is_fixed(P))
    fused_lr = sorted(P for P in pp.MIX_THREADS if P % 2 == 0 and P // 2 not in ls.SMOOTH_EXCLUDED and ls.mixed_is_fixed(P))
    assert sorted(P for P, real in ends if real) == fused_real == [512, 800, 1024, 1600, 2205, 2400, 3200, 4096, 4410, 4800, 8820, 9600]
    assert sorted(P for P, real in ends if not real) == fused_lr == [800, 1024, 1600, 2048, 2400, 3200, 4410, 4800, 8192, 8820, 9600, 17640, 19200]
    assert all(pair is not None for pair in ends.values())


def test_the_dead_inequalities_cannot_bind():
    # samples <= 3072 (and with it samples < 65536 and the 16-bit row words): at NT 256 the image fits four times with either tail, so
    # M + 1 + samples <= (40960 - 2048) / 8 = 4864; samples <= R + M - 1 (test_row_tables_are_the_oracles) and R <= 1024
    assert (pp.LDS_CAP // 4 - min(pp.SEEDED_TAIL, pp.generic_tail(2))) // 8 == 4864
    for M in range(1, 4864):
        if M + 1 + (pp.IN_REGS_SAMPLES + 1) <= 4864:
            assert 1024 + M - 1 <= pp.IN_REGS_SAMPLES
    # ... and over the search range: the widest axes at every window whose image could fit four times
    for W in list(range(8, 2400, 97)) + [2048, 2049, 2400, 2432]:
        for f_min, f_max in ((0.01, 1.0e6), (32.0, 24000.0), (1.0, 1.0e5), (20.0, 96000.0)):
            for rows in (1024, 1000, 512):
                for pal in (pp.SEQ256, pp.RAMP7):
                    c = pp.Config(W=W, f_min=f_min, f_max=f_max, rows=rows, palette=pal)
                    p = pp.predicates(c, pal.n == 256)
                    if p.get("nt") == 256:
                        assert p["samples<=3072"] and p["samples<65536"] and p["words<65536"], c
    # the 16-bit words of the fused 4096-point path: a row has at most M - 1 samples
    for f_min, f_max, rows in ((0.01, 1.0e6, 1), (0.01, 1.0e6, 1024), (32.0, 24000.0, 2), (1.0, 1.0e5, 7)):
        assert pp.wg_predicates(pp.Config(f_min=f_min, f_max=f_max, rows=rows))["wg words"]
    # ten bins per thread: every compile-time plan, both modes
    for P, nt in pp.MIX_THREADS.items():
        assert P // 2 - 1 <= nt * 10, P
        if P <= ls.MIX_MAX_P // 2:
            assert P // 2 <= pp.MIX_REAL_THREADS.get(P, nt) * 10, P
    for c in pp.sweep():
        p = pp.mixed_predicates(c.cfg)
        assert p.get("real W/2<=10nt", True) and p.get("mixed M<=10nt", True), c.name


def test_the_two_members_of_a_pair_differ_in_exactly_their_inequality():
    for p in _all_pairs():
        a, b = pp.all_predicates(p.a.cfg, p.a.seeded), pp.all_predicates(p.b.cfg, p.b.seeded)
        assert a[p.target] is True and b[p.target] is False, p.a.name
        for k in set(a) | set(b):
            if k != p.target and k not in p.follows:
                assert a.get(k) == b.get(k), (p.a.name, k, a.get(k), b.get(k))
        # the nearest reachable values: neighbouring integers, neighbouring doubles
        if p.knob == "palette":
            assert p.b.cfg.palette.n - p.a.cfg.palette.n == 1
            va = vb = None
        else:
            va, vb = getattr(p.a.cfg, p.knob), getattr(p.b.cfg, p.knob)
            assert abs(va - vb) == 1 if isinstance(va, int) else np.nextafter(va, vb) == vb, p.a.name
        same = {f: getattr(p.a.cfg, f) == getattr(p.b.cfg, f) for f in p.a.cfg.__dataclass_fields__ if f not in (p.knob, "flags")}
        assert all(same.values()), (p.a.name, same)
        # and what the inequality decides differs
        if p.target.startswith("wg "):
            assert pp.wg_fusable(p.a.cfg) and not pp.wg_fusable(p.b.cfg)
            assert pp.render_bits(p.a.cfg, True) == (1, 1) and pp.render_bits(p.b.cfg, True) == (0, 0)
            assert pp.bands_fused(p.a.cfg) == 1 and pp.bands_fused(p.b.cfg) == 0
        elif p.target in ("real column<=160K", "mixed column<=image"):
            assert pp.render_bits(p.a.cfg, True) == (1, 1) and pp.render_bits(p.b.cfg, True) == (0, 0), p.a.name
            assert pp.bands_fused(p.b.cfg) == 0
        elif p.target == "bands tables<=48K":      # launch_render_bands' switch: launch_render's class is the same on both sides
            assert p.a.cls == p.b.cls and pp.bands_tables_in_lds(p.a.cfg.palette.n) and not pp.bands_tables_in_lds(p.b.cfg.palette.n)
        else:
            assert p.a.cls != p.b.cls, p.a.name
    # the counts the issue names at the fused limit jump by two between neighbouring doubles: the pair is the nearest reachable
    assert pp.MAGNITUDE_IN_PAIR == (20480, 20481)
    assert pp.magnitude_in_staged(pp.Config(W=20480)) and not pp.magnitude_in_staged(pp.Config(W=20481))
    assert pp.bands_tables_in_lds(4096) and pp.bands_tables_in_lds(12033) and not pp.bands_tables_in_lds(12034) and not pp.bands_tables_in_lds(40000)


def test_the_named_extras_are_what_their_names_say():
    by_name = {c.name: c for c in pp.sweep()}
    assert [by_name[f"rows {R}"].cfg.rows for R in (1, 255, 256, 257, 1023, 1024, 1025)] == [1, 255, 256, 257, 1023, 1024, 1025]
    assert by_name["rows 65536"].cfg.rows == 65536
    assert pp.row_table(by_name["a row of 255 samples"].cfg).max_count == 255 and pp.row_table(by_name["a row of 256 samples"].cfg).max_count == 256
    assert pp.wg_fusable(by_name["a row of 256 samples"].cfg)            # the row word holds 16 bits of count
    assert pp.row_table(by_name["a row of 256 samples"].cfg).block_max_cnt == 255
    masks = {"single_rows 0000": 0b0000, "single_rows 0011": 0b0011, "single_rows 1111": 0b1111, "single_rows partial last block": 0b111}
    for name, mask in masks.items():
        c = by_name[name].cfg
        assert pp.row_table(c).single_rows == mask and pp.wg_fusable(c), (name, bin(pp.row_table(c).single_rows))
    assert by_name["single_rows partial last block"].cfg.rows % 256
    top = pp.row_table(by_name["f_max far above Nyquist"].cfg).counts
    assert top[-64:] == (1,) * 64 and max(top) > 1                       # the top rows all clamp to the last bin
    low = pp.row_table(by_name["f_min below one bin"].cfg).counts
    assert low[:256] == (1,) * 256
    assert by_name["sample rate 44100.9"].cfg.sr_u32 == 44100
    sizes = sorted({c.cfg.palette.n for c in pp.sweep() if c.cfg.palette.kind == "ramp"})
    assert sizes == [2, 7, 255, 256, 257, 4096, 12033, 12034, 40000, 40705, 40706, 65536]
    for n in (2, 7, 255, 256, 257, 4096, 40000, 65536):
        ctx = [c for c in pp.sweep() if c.group == f"palette-{n}"]
        assert {(c.cfg.palette.stereo, c.cfg.lut_index_mode) for c in ctx} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    assert [pp.render_class(pp.Config(palette=pp.Palette("ramp", "ramp", n)), False) for n in (4096, 40000, 65536)] == \
        [("two_pass", 1024, 8, 0), ("column", False, True), ("column", True, False)]
    assert pp.render_class(pp.Config(palette=pp.Palette("ramp", "ramp", 40705)), False) == ("column", False, True)
    assert pp.render_class(pp.Config(palette=pp.Palette("ramp", "ramp", 40706)), False) == ("column", True, False)
    assert [c.cls for c in pp.sweep() if c.group == "palette-65536-long"] == [("column", False, False)] * 2
    assert {c.cfg.palette.stereo for c in pp.sweep() if c.cfg.palette.kind == "scheme"} == {False, True}
    # windows: every class has its window, kernel 11's long windows take no stream
    assert all(pp.needs_large(c.cfg.W) == ("large_transforms" in c.cfg.flags) for c in pp.sweep())
    # the buffer of made magnitudes stays under 128 MiB on a 256-CU device
    for c in pp.sweep():
        blocks = pp.blocks_launched(c.cfg, c.seeded, 256)
        cols = min(2 * blocks + 3, (128 << 20) // (c.cfg.M * 8))
        assert cols >= 10 and cols * c.cfg.M * 8 <= 128 << 20, c.name


def test_the_dB_ranges_fall_clearly_on_either_side_of_the_seed_proof():
    # passing: the default range, its switch points within a small fraction of an index of the seed's line, no level skipped
    margin, skipped = pp.seed_margin(-70.0, -10.0)
    assert skipped == 0 and margin < 0.1, (margin, skipped)
    # failing: the narrow span holds fewer float32 dB values than the palette has levels, so levels are skipped -- two neighbouring
    # switch points coincide and the seed's line cannot pass within half an index of both
    lo, hi = np.float32(pp.NARROW_DB[0]), np.float32(pp.NARROW_DB[1])
    values = (int(np.float32(-hi).view(np.uint32)) - int(np.float32(-lo).view(np.uint32))) * -1 + 1
    assert 0 < values < 255, values
    margin, skipped = pp.seed_margin(*pp.NARROW_DB)
    assert skipped >= 255 - values and margin >= 0.5, (margin, skipped)
    # failing: levels above the dB of FLT_MAX (about +385) are unreachable
    db_of_max = 10.0 * np.log10(float(np.finfo(np.float32).max))
    assert 385.0 < db_of_max < 386.0 and (db_of_max + 70.0) / 470.0 * 256 < 255
    for name in ("proof fails: unreachable top levels", "proof fails: narrow span"):
        c = [c for c in pp.sweep() if c.name == name][0]
        assert c.proof is False and not c.seeded and pp.render_bits(c.cfg, c.proof) == (1, 0)
