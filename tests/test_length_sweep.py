"""The length sets of tests/length_sweep.py (what tests/test_gpu_lengths.py runs on the GPU) checked on the CPU: their sizes, that they
cover what they are for -- every (RA, RB) stage case and every stage count of the mixed-radix plans, every N1 and every N2 of kernel 11's
direct plans, every exact fit of a chirp-z convolution -- that no length is run twice, and that the truth of the longest is affordable."""
import collections
import time

import numpy as np

import edge_signals as es
import length_sweep as ls



def test_smooth_is_every_smooth_window_but_those_of_other_kernels():
    assert len(ls.ALL_SMOOTH_W) == 339
    assert ls.SMOOTH_EXCLUDED == [4, 8, 16, 32, 64, 128, 256, 2048, 8192]
    windows = [e.W for e in ls.SMOOTH if not e.flags]
    assert len(windows) == len(set(windows)) == 339 - len(ls.SMOOTH_EXCLUDED)
    assert [e.key for e in ls.SMOOTH if e.flags] == [(2400, ("mixed_generic",))] and len(ls.SMOOTH) == 339 - len(ls.SMOOTH_EXCLUDED) + 1
    assert all(ls.smooth7(2 * e.W) and 4 <= e.W <= 10240 for e in ls.SMOOTH)
    # the route: kernel 9 at the application's window only; the compile-time plans are those of the macros, W 1200 included (2W = 2400)
    assert [e.W for e in ls.SMOOTH if e.kernel == 9] == [2400] and all(e.kernel in (6, 9) for e in ls.SMOOTH)
    fixed = sorted(e.W for e in ls.SMOOTH if e.bit2 and not e.flags)
    assert fixed == [400, 512, 800, 1024, 1200, 1600, 2205, 2400, 4096, 4410, 4800, 8820, 9600]
    assert [e.W for e in ls.SMOOTH if not e.bit3_mono] == [5, 6, 7]      # no W-point plan of real-input mode below W 8
    # the routes tests/edge_signals.py pins by name agree
    by_key = {e.key: e for e in ls.SMOOTH}
    for r in es.ROUTES:
        flags = tuple(f for f in r.flags if f == "mixed_generic")
        e = by_key.get((r.W, flags))
        if e is None or r.kernel not in (6, 9) or set(r.flags) - {"mixed_generic"}:
            continue
        on, off = e.bits(min(r.channels, 2))
        assert e.kernel == r.kernel and on & r.bits_clear == 0 and off & r.bits_set == 0, r.name


def test_fixed_plan_table_is_the_macros():
    plans = {}
    for row in ls.macro("MIX_FIXED_PLANS") + ls.macro("MIX_FIXED4_PLANS"):
        P, ab = row[0], row[1:-1]
        plans[P] = tuple(zip(ab[0::2], ab[1::2]))
    assert plans == ls.MIX_FIXED
    # every compiled plan is the run-time rule's, so every one of them is reached (as a 2W-point or as a W-point plan)
    for P, plan in plans.items():
        assert tuple(ls.mixed_radix_plan(P)) == plan, P


def test_every_stage_case_and_every_stage_count_occurs():
    cases = set(ls.macro("MIX_STAGE_CASES"))
    asked, counts = set(), collections.Counter()
    for W in ls.ALL_SMOOTH_W:                       # what any plan of any served window asks for
        for plan in (ls.mixed_radix_plan(2 * W), ls.mixed_radix_plan(W)):
            asked.update(plan)
            counts[len(plan)] += 1
    assert dict(counts) == {1: 22, 2: 131, 3: 351, 4: 172, 5: 2}
    assert asked <= cases
    run, stages = set(), set()
    for e in ls.SMOOTH:
        for plan in (e.plan, e.plan_mono):
            run.update(plan)
            if plan:
                stages.add(len(plan))
    assert stages == {1, 2, 3, 4, 5}
    # stage cases only the excluded powers of two would ask for are nobody's on the mixed-radix route
    excluded = set()
    for W in ls.SMOOTH_EXCLUDED:
        excluded.update(ls.mixed_radix_plan(2 * W))
    assert asked - run <= excluded and asked - run == set(), asked - run
    # every R_last the padding rule sees, padded and unpadded
    pads = {(e.plan[-1][0] * e.plan[-1][1], ls.mixed_pad_every(2 * e.W, e.plan) != 0) for e in ls.SMOOTH}
    assert {r for r, _ in pads} == {3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16, 20, 21, 25, 28}
    assert all((r, True) in pads and (r, False) in pads for r in (4, 8, 10, 14, 16, 20)) and not any(p for r, p in pads if r % 2)


def test_pow2_routes():
    assert sorted({e.W for e in ls.POW2}) == [1 << k for k in range(2, 14)]
    assert sorted(e.W for e in ls.POW2 if e.flags == ("force_generic",)) == [1 << k for k in range(2, 14)]
    assert sorted(e.W for e in ls.POW2 if not e.flags) == ls.SMOOTH_EXCLUDED
    assert {e.W for e in ls.POW2} - set(ls.SMOOTH_EXCLUDED) <= {e.W for e in ls.SMOOTH}   # 512, 1024, 4096: the default route is SMOOTH's
    assert all(e.kernel == 0 for e in ls.POW2 if e.flags == ("force_generic",) or (not e.flags and e.W <= 256))
    assert {(e.W, e.kernel) for e in ls.POW2 if not e.flags and e.W > 256} == {(2048, 2), (8192, 10)}


def test_chirp_classes_and_exact_fits():
    default = {e.W: e for e in ls.CHIRP if not e.flags}
    assert all(ls.chirp_served(W) for W in default)
    for W in (11, 43, 171, 683, 2731):
        assert 3 * W - 1 == ls.chirp_length(W) and W in default, W
    for W in (683, 2731):                           # ... and of the mono real-input convolution over ceil(W / 2) pairs
        assert W + (W + 1) // 2 - 1 == ls.chirp_length_mono(W)
    # every class of the (l, r) convolution from 32 on and every class of the mono convolution is run at both ends
    for L in ls.CHIRP_CLASSES[1:]:
        members = sorted(W for W in default if ls.chirp_length(W) == L)
        last = max(W for W in range(4, 5462) if ls.chirp_length(W) == L and ls.chirp_served(W))
        first = min(W for W in range(4, 5462) if ls.chirp_length(W) == L and ls.chirp_served(W))
        assert members[0] == first and members[-1] == last, (L, members)
        if L >= 128:
            assert sum(W % 2 for W in members) >= 2 and sum(1 - W % 2 for W in members) >= 2, (L, members)
    assert not [W for W in range(4, 6) if ls.chirp_served(W)]           # the class L = 16 holds W 4 and 5: both smooth
    for L in ls.CHIRP_MONO_CLASSES:
        served = [W for W in range(86, 5462) if ls.chirp_length_mono(W) == L and ls.chirp_served(W)]
        members = sorted(W for W, e in default.items() if e.L_mono == L)
        assert members[0] == served[0] and members[-1] == served[-1] and len(members) >= 6, (L, members)
    assert [max(W for W in range(86, 5462) if ls.chirp_length_mono(W) == L) for L in ls.CHIRP_MONO_CLASSES] == [342, 683, 1366, 2731, 5461]
    # the ladder: every window below 86, and the class ends of the composite stages under force_generic
    assert all(e.ladder == (e.W < 86 or e.flags == ("force_generic",)) for e in ls.CHIRP)
    assert all(e.bit2 != e.ladder and e.bit3_mono != e.ladder and e.kernel == 4 for e in ls.CHIRP)
    forced = {e.W for e in ls.CHIRP if e.flags}
    assert forced >= {86, 171, 172, 683, 2731, 5461} and all(W >= 86 for W in forced)


def test_large_direct_covers_every_sub_transform_length():
    assert len(ls.LARGE_DIRECT_ALL) == 944
    plans = [es.large_plan(W) for W in ls.LARGE_DIRECT_ALL]
    n1, n2 = {p[1] for p in plans}, {p[2] for p in plans}
    assert len(n1) == 115 and len(n2) == 121 and len(n1 | n2) == 127
    assert {e.plan[1] for e in ls.LARGE_DIRECT} == n1 and {e.plan[2] for e in ls.LARGE_DIRECT} == n2
    assert len(ls.LARGE_DIRECT) == 229 and ls.LARGE_DIRECT[-1].W == 1 << 20
    assert 1.25e8 < sum(2 * e.W for e in ls.LARGE_DIRECT) < 1.27e8
    assert all(e.W > 10240 and ls.smooth7(2 * e.W) for e in ls.LARGE_DIRECT)


def test_large_chirp_classes_and_exact_fits():
    ws = [e.W for e in ls.LARGE_CHIRP]
    for W in (10923, 43691, 174763, 699051):
        assert 3 * W - 1 == ls.chirp_length(W) and W in ws, W
    assert all(ls.large_chirp_served(W) and es.large_plan(W)[3] for W in ws)
    for L in ls.LARGE_CHIRP_CLASSES:
        members = [e.W for e in ls.LARGE_CHIRP if e.L == L]
        assert len(members) == 2 and (ls.chirp_length(members[0] - 1) < L or members[0] - 1 == 5461), (L, members)
    assert ws[0] == 5462 and ws[-1] == (1 << 20) - 1


def test_no_length_is_run_twice():
    keys = collections.Counter(e.key for s in ls.SETS.values() for e in s)
    assert max(keys.values()) == 1, [k for k, n in keys.items() if n > 1]
    # a window lies in one set only -- but the powers of two 512, 1024 and 4096, which SMOOTH runs by default and POW2 under its flags
    sets_of = collections.defaultdict(set)
    for name, s in ls.SETS.items():
        for e in s:
            sets_of[e.W].add(name)
    assert {W for W, names in sets_of.items() if len(names) > 1} == {512, 1024, 4096}
    # every entry lies in exactly one chunk
    chunks = ls.chunks()
    assert sorted(e.key for run in chunks.values() for e in run) == sorted(keys)
    assert all(chunks.values())


def test_local_peak_at_is_the_inverse_tests_local_peak():
    from test_gpu_istft import local_peak
    rng = np.random.default_rng(3)
    for ch in (1, 2):
        x = rng.standard_normal((700, ch)).astype(np.float32)
        for W, lo, hi in ((100, 99, 105), (37, 0, 700), (300, 299, 304)):
            assert np.array_equal(ls.local_peak_at(x, W, lo, hi), local_peak(x.astype(np.float64), W)[lo:hi])


def test_truth_of_the_longest_lengths_is_affordable():
    longest = max(e.W for s in ls.SETS.values() for e in s)
    assert longest == 1 << 20
    for W in (longest, longest - 1, 699051):       # the longest power of two, the longest chirp-z length, the longest exact fit
        lr = np.ones((W, 2), np.float32)
        t0 = time.perf_counter()
        es.truth_frame(lr, W)
        dt = time.perf_counter() - t0
        print(f"truth of W {W}: {dt:.2f} s")
        assert dt < 5.0, (W, dt)


def test_independent_float32_transform_reads_below_the_bound_on_noise():
    # the yardstick of a finding (a length above its bound): an independent float32 FFT of white noise stays under 1 x the wide floor
    for e in (ls.SMOOTH[40], ls.CHIRP[30]):
        x = ls.stream(e, 2, 1)
        r = ls.independent_float32_ratio(x[:e.W], e.W, e.floor)
        assert 0.0 < r < 1.0, (e.W, r)
