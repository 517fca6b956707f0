"""The job splits of every persistent launch, restated in tests/cu_counts.py, proved on the CPU: at every compute-unit count every job
index lies inside its range and every job is done exactly once.  First for every (case, limit) of the table tests/test_gpu_cu_counts.py
runs -- this is why that table cannot address a row outside its buffers -- then over an exhaustive small grid, and last the check of the
checker: two broken models must fail the same properties.

What the sweep costs.  n_cu 1 .. 40, 255 and 256; pairs 1 .. 5 and 8; H 512 (slide) and 300; job counts 1 .. 3 * 8 * n_cu + 5, thinned:
every frame count up to 2 n_cu / pairs + 8 (two workgroups' worth and the short launches) and two on either side of 1, 2, 3, 7, 8, 9, 15,
16, 17, 23 and 24 times n_cu / pairs, rounded up -- where xcds switches (n_jobs >= 8 blocks) and jobs_per_xcd and run_len change their rounding -- and
the last three; at 255 and 256 CUs the first 40 counts and one on either side.  Paired mono frames from an even and an odd first_frame.
That is about 40 000 walks of 300 jobs on average: the whole file takes about 45 s of plain Python on one core (3.5 s each for the four
cases at 255 and 256 CUs, under 1 s for every other)."""
import itertools

import pytest

import bounds_arena as ba
import cu_counts as cc

N_CU = list(range(1, 41)) + [255, 256]
PAIRS = [1, 2, 3, 4, 5, 8]


KS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24)      # multiples of the workgroup count around which xcds and the roundings change


def thinned(limit: int, unit: int, dense: int, around: int = 2, per: int = 1) -> list:
    """1 .. dense in full, then `around` on either side of ceil(k unit / per) for the multiples k of KS, and the last three up to `limit`"""
    out = set(range(1, min(dense, limit) + 1))
    for k in KS:
        centre = -(-k * unit // per)
        out.update(range(max(centre - around, 1), min(centre + around, limit) + 1))
    out.update(range(max(limit - 2, 1), limit + 1))
    return sorted(out)


def check_run_split(n_cu, n_jobs, per_cu, what):
    per, blocks = cc.run_split(n_cu, n_jobs, per_cu)
    assert per >= 1 and blocks <= n_cu * per_cu, (what, "more workgroups than the split (and the peak partial columns) allow")
    walk = cc.run_walk(per, blocks, n_jobs)
    assert [j for w in walk for j in w] == list(range(n_jobs)), (what, "not exactly once")
    assert all(w for w in walk), (what, "an empty run")
    return per, blocks


def forward_problems(r, n_cu, first, n):
    split = cc.forward_split(r, n_cu, first, n)
    if split[0] == "k16":
        return cc.k16_problems(split[1])
    _, per, blocks, frames = split
    per_cu = cc.run_split_per_cu(r)
    bad = []
    if blocks > n_cu * per_cu:
        bad.append(("more workgroups than the split allows", blocks))
    jobs = [j for w in cc.run_walk(per, blocks, len(frames)) for j in w]
    if jobs != list(range(len(frames))):
        bad.append(("jobs not exactly once",))
    if sorted(f for j in jobs for f in frames[j]) != list(range(n)):
        bad.append(("frames not exactly once",))
    return bad


@pytest.mark.parametrize("case", cc.TABLE, ids=lambda c: c.name)
def test_gpu_table_every_job_exactly_once_and_in_range(case):
    r = cc.route_of(case)
    for limit in cc.LIMITS:
        n_cu = cc.limit_value(limit, cc.CPU_DEVICE_CU)
        F = cc.frames_at(case, limit)
        if case.kind == "forward":
            for first, n in cc.forward_calls(case, limit):
                assert n >= 1 and forward_problems(r, n_cu, first, n) == [], (case.name, limit, first, n)
                if cc.run_split_per_cu(r) == 4 and not r.paired:       # the fused peak route: runs lengthened to whole columns
                    fpj = cc.peak_fpj(r)
                    for group in (3, cc.peak_run_group(r, n, n_cu)):
                        n_jobs = (n + fpj - 1) // fpj
                        per, _ = cc.run_split(n_cu, n_jobs, 4)
                        per, blocks = cc.runs_of(n_jobs, cc.ba.peak_align_run(per, fpj, min(group, n)))
                        assert blocks <= n_cu * 4, (case.name, limit, group, "partial columns of more workgroups than the buffer holds")
                        assert [j for w in cc.run_walk(per, blocks, n_jobs) for j in w] == list(range(n_jobs))
        elif case.kind == "pixel":
            for n, per_cu in itertools.product((F, F - case.first), range(1, 9)):
                assert cc.pixel_problems(cc.pixel_blocks(n_cu, per_cu, n * r.pairs), n * r.pairs) == [], (case.name, limit, n, per_cu)
        else:
            N = (F - 1) * r.H + r.W
            for (s0, s1), per_cu in itertools.product(((0, N), (case.first, N), (case.first, case.first + r.H + 1)), range(1, 17)):
                assert cc.istft_problems(cc.istft_split(n_cu, per_cu, r.pairs, r.W, r.H, s0, s1)) == [], (case.name, limit, s0, s1, per_cu)


def test_the_windows_of_the_sweep_hold_the_counts_where_xcds_switches():
    # n_cu = 40, pairs = 3: xcds turns 8 at the first n_frames with 3 n_frames >= 8 * 40, 107 -- not at 8 * (40 // 3) = 104
    counts = thinned(-(-(3 * 8 * 40 + 5) // 3), 40, 2 * 40 // 3 + 8, 2, per=3)
    assert 106 in counts and 107 in counts
    assert cc.k16_launch(40, 106, 3, 300).xcds == 1 and cc.k16_launch(40, 107, 3, 300).xcds == 8
    for n_cu, pairs in itertools.product((8, 16, 24, 40, 256), PAIRS):   # (the counts whose workgroups split into 8 XCDs)
        flip = -(-8 * n_cu // pairs)
        counts = thinned(-(-(3 * 8 * n_cu + 5) // pairs), n_cu, 40 if n_cu > 40 else 2 * n_cu // pairs + 8, 1 if n_cu > 40 else 2, per=pairs)
        assert flip - 1 in counts and flip in counts, (n_cu, pairs)
        assert (cc.k16_launch(n_cu, flip - 1, pairs, 300).xcds, cc.k16_launch(n_cu, flip, pairs, 300).xcds) == (1, 8), (n_cu, pairs)


def test_pixel_cases_cover_the_launch_render_classes():
    import pixel_plans as pp
    seen = set()
    for case in cc.TABLE:
        if case.kind != "pixel":
            continue
        r = cc.route_of(case)
        cfg = pp.Config(W=r.W, channels=r.channels)
        got = (pp.render_class(cfg, True), pp.blocks_launched(cfg, True, 1))
        assert got == cc.PIXEL_CLASSES[case.name], (case.name, got)
        seen.add(got)
    assert len(seen) == 7 and {c[0][1] for c in seen if c[0][0] == "two_pass"} == {256, 512, 1024}
    assert {c[1] for c in seen if c[0][0] == "two_pass"} == {1, 2, 4, 8} and (("column", True, True), 8) in seen


def test_gpu_table_reaches_every_branch():
    reached = set()
    for case, limit in itertools.product(cc.TABLE, cc.LIMITS):
        reached |= cc.branches(case, limit, cc.CPU_DEVICE_CU)
    assert reached <= set(cc.REQUIRED_BRANCHES), reached - set(cc.REQUIRED_BRANCHES)
    assert not set(cc.REQUIRED_BRANCHES) - reached, sorted(set(cc.REQUIRED_BRANCHES) - reached)


def test_the_bank_kinds_reach_a_last_job_without_its_second_frame():
    """the filterbank calls ride the forward cases of the 4096-point kernels; the fused ones on the real-input rows meet, at low limits, a run
    of several jobs whose last job holds one frame (the split is the rows' own launcher's: proved above for every case and limit)"""
    assert {c.name: cc.bank_kinds(cc.route_of(c)) for c in cc.TABLE if c.kind == "forward" and cc.bank_kinds(cc.route_of(c))} == {
        "k1r_h256": ("fbank",), "k1r_h100": ("fbank",), "k1r_h256_align4": ("fbank",), "k1_complex_mono": ("fbank",), "k1_paired_mono": ("fbank",),
        "k1_lr_h256": ("fbank", "fbank_cross"), "k1_lr_h58": ("fbank", "fbank_cross"), "k1_ch4": ("fbank", "fbank_cross"),
        "k1_ch8": ("fbank", "fbank_cross")}
    reached = cc.bank_cases_with_a_last_job_of_one_frame(cc.CPU_DEVICE_CU)
    assert {name for name, _ in reached} == {"k1r_h256", "k1r_h100", "k1r_h256_align4"}
    # 75 frames are 38 jobs, the last of one frame; the sub-range from frame 3 is 72 frames: no such job.  At limits 1 .. 8 the last workgroup
    # runs that job behind others
    assert {limit for name, limit in reached if name == "k1r_h256"} >= {1, 2, 3, 5, 8}


def test_the_welch_kinds_ride_every_forward_case():
    """sgx_psd_batch at group 3 behind the rows of every forward case, sgx_csd_batch wherever the case has an (l, r) pair: the split under
    test is the rows' own (proved above for every case and limit), and at group 3 every case has a ragged last column or several columns"""
    forward = [c for c in cc.TABLE if c.kind == "forward"]
    assert forward
    for c in forward:
        r = cc.route_of(c)
        assert cc.welch_kinds(r) == (("psd_3", "csd_3") if r.channels >= 2 else ("psd_3",)), c.name
        for limit in cc.LIMITS:
            for first, n in cc.forward_calls(c, limit):
                assert n >= 4, (c.name, limit, first, n)          # at least two columns of three frames
                # one range of whole columns at these sizes: the seams of the ranges are tests/test_gpu_psd.py's and test_gpu_bounds.py's
                for cross in (False, True)[:len(cc.welch_kinds(r))]:
                    plan = ba.welch_ranges(r.W, r.pairs, cross, n, 3, True)
                    assert not plan.carried and not plan.piece and len(plan.ranges) == 1, (c.name, limit, first, n)
    assert {len(cc.welch_kinds(cc.route_of(c))) for c in forward} == {1, 2}


@pytest.mark.parametrize("n_cu", N_CU)
def test_sweep_16384_point_walk(n_cu):
    big = n_cu > 40
    for pairs in PAIRS:
        top = -(-(3 * 8 * n_cu + 5) // pairs)
        for n_frames in thinned(top, n_cu, 40 if big else 2 * n_cu // pairs + 8, 1 if big else 2, per=pairs):
            for H in (512, 300):
                L = cc.k16_launch(n_cu, n_frames, pairs, H)
                assert L.blocks <= n_cu and cc.k16_problems(L) == [], (n_cu, pairs, n_frames, H)
    top = 2 * (3 * 8 * n_cu + 5)
    for n_frames, first in itertools.product(thinned(top, 2 * n_cu, 40 if big else 4 * n_cu + 8, 1 if big else 2), (0, 1)):   # frame pairs by global index
        L = cc.k16_launch(n_cu, n_frames, 1, 512, paired_mono=True, first_frame=first)
        assert L.blocks <= n_cu and cc.k16_problems(L) == [], (n_cu, n_frames, first)


@pytest.mark.parametrize("n_cu", N_CU)
def test_sweep_run_split_pixels_and_inverse(n_cu):
    big = n_cu > 40
    top = 3 * 8 * n_cu + 5
    for per_cu, n_jobs in itertools.product((3, 4), thinned(top, n_cu, 40 if big else 4 * 4 * n_cu + 8)):
        check_run_split(n_cu, n_jobs, per_cu, (n_cu, per_cu, n_jobs))
    for n_frames, first in itertools.product(thinned(top, n_cu, 64), (0, 1)):    # frame pairs by global index, real-input frame pairs
        base, n_jobs = cc.paired_jobs(first, n_frames)
        assert sorted(f for j in range(n_jobs) for f in cc.paired_frames_of(j, base, first, n_frames)) == list(range(n_frames))
        assert sorted(f for j in range((n_frames + 1) // 2) for f in cc.real_frames_of(j, n_frames)) == list(range(n_frames))
    for per_cu, n_columns in itertools.product((1, 2, 3, 8, 11), thinned(top, n_cu, 40 if big else 3 * n_cu + 8)):
        assert cc.pixel_problems(cc.pixel_blocks(n_cu, per_cu, n_columns), n_columns) == [], (n_cu, per_cu, n_columns)
    for per_cu, pairs, (W, H), n in itertools.product((1, 2, 5), (1, 3, 4), ((2048, 256), (2400, 93), (1102, 1500)), thinned(top, n_cu, 40)):
        N = (n - 1) * H + W
        for s0, s1 in ((0, N), (H + 1, N), (N - 1, N)):
            assert cc.istft_problems(cc.istft_split(n_cu, per_cu, pairs, W, H, s0, s1)) == [], (n_cu, per_cu, pairs, W, H, s0, s1)


# ---- the check of the checker -----------------------------------------------------------------------------------------------------------
def test_a_walk_without_the_carry_fails_the_proof():
    # pairs = 3, five workgroups: job_step = 5 = 1 hop + 2 pairs, the carry is due on every second step
    L = cc.k16_launch(5, 43, 3, 1024)
    assert not L.slide and L.blocks == 5 and cc.k16_problems(L) == []
    bad = cc.k16_problems(L, carry=False)
    assert any(b[0] == "not exactly once" for b in bad) and any(b[0] == "(hop, pair) is not divmod(job, pairs)" for b in bad), bad
    # ... and on a case of the GPU table: every (case, limit) whose job_step is no multiple of the pairs, with more than one job
    failing = 0
    for case, limit in itertools.product(cc.TABLE, cc.LIMITS):
        if case.kind != "forward" or cc.route_of(case).kernel != 10:
            continue
        r, n_cu = cc.route_of(case), cc.limit_value(limit, cc.CPU_DEVICE_CU)
        first, n = cc.forward_calls(case, limit)[0]
        L = cc.k16_launch(n_cu, n, r.pairs, r.H, r.paired, first)
        needs_carry = not L.slide and not L.mono and (L.blocks // L.xcds) % L.pairs != 0 and cc.more_than_one_job(case, limit, cc.CPU_DEVICE_CU, "k16")
        assert bool(cc.k16_problems(L, carry=False)) == needs_carry, (case.name, limit)
        failing += needs_carry
    assert failing >= 3


def test_a_floored_run_length_fails_the_proof():
    # 75 jobs on 4 workgroups: per = 18 leaves jobs 72 .. 74 undone
    per, blocks = cc.run_split(1, 75, 4, floor_per=True)
    assert (per, blocks) == (18, 4)
    assert [j for w in cc.run_walk(per, blocks, 75) for j in w] != list(range(75))
    assert check_run_split(1, 75, 4, "the real split") == (19, 4)
    # ... everywhere the job count is no multiple of the workgroups
    for n_cu, n_jobs in itertools.product((1, 2, 3, 5, 8, 9, 16, 32), (37, 38, 75, 76)):
        per, blocks = cc.run_split(n_cu, n_jobs, 4, floor_per=True)
        done = [j for w in cc.run_walk(per, blocks, n_jobs) for j in w]
        assert (done == list(range(n_jobs))) == (n_jobs <= n_cu * 4 or n_jobs % (n_cu * 4) == 0), (n_cu, n_jobs)


def test_the_omit_only_variants_are_predicted_by_the_model():
    # skipping the walk's last step leaves exactly the rows of the last step unwritten, and only where a workgroup has more than one job
    L = cc.k16_launch(8, 33, 4, 300)
    assert L.xcds == 8
    full = [s for b in range(L.blocks) for s in cc.k16_walk(L, b).steps]
    cut = [s for b in range(L.blocks) for s in cc.k16_walk(L, b, skip_last_step=True).steps]
    assert set(cut) < set(full) and len(full) - len(cut) == sum(len(cc.k16_walk(L, b).steps) > 1 for b in range(L.blocks))
    # the limit-0 references of the GPU table give no workgroup a second job: a variant library computes them in full
    assert cc.references_have_one_job(cc.CPU_DEVICE_CU, "run_split") and cc.references_have_one_job(cc.CPU_DEVICE_CU, "k16")
    one = cc.k16_launch(256, 33, 4, 300)
    assert [cc.k16_walk(one, b).steps for b in range(one.blocks)] == [cc.k16_walk(one, b, skip_last_step=True).steps for b in range(one.blocks)]
