"""How every persistent launch deals its jobs from the compute-unit count in force (a plain helper of tests/test_cu_counts.py and
tests/test_gpu_cu_counts.py: no GPU, no torch).

The launchers size their grids from sgx_ctx::n_cu (sgx_set_cu_limit; default the device's own count) and the kernels walk their jobs from
blockIdx / gridDim.  Both are restated here from the sources, nothing asks the library:

  run_split / runs_of (csrc/sgx_internal.hpp)          the 4096-point kernels (4 workgroups per CU), the 4800-point kernel (3 per CU):
                                                       workgroup b runs jobs [b per, min((b + 1) per, n_jobs))
  launch_w16384 (csrc/stft16384_w.hip)                 blocks, xcds, jobs_per_xcd, slide, run_len ...
  stft16384_w_kernel, "Job order"                      ... and the walk itself: wg, job_begin, job_end, job_step, and (hop_c, pair_c) advanced
                                                       by (step_hops, step_pairs) with the carry from pair to hop, as the loop's head does it
  render_two_pass_kernel (csrc/sgx_kernels.hip)        columns blockIdx.x, + gridDim.x, ...; the columns requested one and two strides ahead
  launch_istft / istft_kernel (csrc/stft_istft.hip)    groups of `run` hop blocks, a run at least kw + 1 blocks (its warm-up is kw blocks)

TABLE is the case table of tests/test_gpu_cu_counts.py; tests/test_cu_counts.py proves on the CPU, before anything runs on a GPU, that at
every (case, limit) every job index lies inside its range and every job is done exactly once.  branches() names which branch of the above
a (case, limit) takes; the GPU test asserts that the table reaches every name in REQUIRED_BRANCHES.

Two quantities the launchers take from hipOccupancyMaxActiveBlocksPerMultiprocessor (the pixel kernel's and the inverse's workgroups per
CU) are parameters here: the properties are proved for every value from 1 to 8 (the pixel launcher's own cap) resp. 1 to 16, and the
branch table claims a branch only where every such value takes it."""
from __future__ import annotations

from dataclasses import dataclass

import bounds_arena as ba
import edge_signals as es
from conftest import FLOOR_K16

XCD_HINT = 8            # stft16384_w.hip kXcdHint
LIMITS = (0, 1, 2, 3, 5, 8, 9, 16, 32, -1)   # 0: the device's own count (the reference); -1: the device's count minus one
CPU_DEVICE_CU = 256     # the count the CPU proof takes for "the device's own": an MI355X in SPX mode


def limit_value(limit: int, device_cu: int) -> int:
    """the n_cu in force for an entry of LIMITS"""
    return device_cu if limit == 0 else device_cu - 1 if limit == -1 else limit


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ---- run_split ---------------------------------------------------------------------------------------------------------------------------
def runs_of(n_jobs: int, per: int):
    return per, ceil_div(n_jobs, per)


def run_split(n_cu: int, n_jobs: int, per_cu: int, floor_per: bool = False):
    """(per, blocks).  floor_per: the broken model of the check of the checker -- `per` rounded DOWN, the grid still the n_cu * per_cu
    workgroups the split was made for (runs_of cannot be kept: it would cover the jobs with more workgroups than the split allows)"""
    blocks = n_cu * per_cu
    if floor_per:
        per = max(n_jobs // blocks, 1)
        return per, min(blocks, ceil_div(n_jobs, per))
    return runs_of(n_jobs, max(ceil_div(n_jobs, blocks), 1))


def run_walk(per: int, blocks: int, n_jobs: int) -> list:
    """the jobs of every workgroup of a run_split kernel: job_begin = blockIdx.x * per, job_end = min(job_begin + per, n_jobs)"""
    return [list(range(b * per, min((b + 1) * per, n_jobs))) for b in range(blocks)]


def paired_jobs(first_frame: int, n_frames: int):
    """(pair_base, n_jobs) of a mono stream whose frames share transforms by GLOBAL index (2q, 2q + 1)"""
    return first_frame // 2, (first_frame + n_frames + 1) // 2 - first_frame // 2


def paired_frames_of(job: int, pair_base: int, first_frame: int, n_frames: int) -> list:
    """the output frames (relative to first_frame) job writes: f0 = 2 (pair_base + job) - first_frame where f0 >= 0, f0 + 1 where it
    is below n_frames"""
    f0 = 2 * (pair_base + job) - first_frame
    return [f for f in (f0, f0 + 1) if 0 <= f < n_frames]


def real_frames_of(job: int, n_frames: int) -> list:
    """stft4096_real.hip: job j is frames (2j, 2j + 1) of the CALL; the last job of an odd count drops the absent second frame"""
    return [f for f in (2 * job, 2 * job + 1) if f < n_frames]


# ---- the 16384-point launcher and its kernel's walk ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class K16Launch:
    mono: bool          # frame pairs of a mono stream (MONO instantiation)
    slide: bool
    pairs: int
    n_frames: int
    first_frame: int
    pair_base: int
    n_jobs: int
    blocks: int
    xcds: int
    jobs_per_xcd: int
    run_len: int
    runs_cap: int       # n_cu / pairs (slide), else 0
    runs_rem: int       # n_cu % pairs (slide), else 0


def k16_launch(n_cu: int, n_frames: int, pairs: int, H: int, paired_mono: bool = False, first_frame: int = 0) -> K16Launch:
    """launch_w16384 from `persistent workgroups, one per CU` on (n_frames >= 1: the launcher returns before for none)"""
    mono = paired_mono
    pair_base, n_jobs = paired_jobs(first_frame, n_frames) if mono else (0, n_frames * pairs)
    blocks = min(n_cu, n_jobs)
    xcds = XCD_HINT if blocks % XCD_HINT == 0 and n_jobs >= XCD_HINT * blocks else 1
    group = 1 if mono else pairs
    jobs_per_xcd = ceil_div(ceil_div(n_jobs, xcds), group) * group
    slide = not mono and H == 512 and pairs <= n_cu
    run_len = runs_cap = runs_rem = 0
    if slide:
        runs_cap, runs_rem = n_cu // pairs, n_cu % pairs
        runs = min(runs_cap, n_frames)
        run_len = ceil_div(n_frames, runs)
        runs = ceil_div(n_frames, run_len)
        blocks = runs * pairs
        xcds = XCD_HINT if blocks % XCD_HINT == 0 else 1
    return K16Launch(mono, slide, pairs, n_frames, first_frame, pair_base, n_jobs, blocks, xcds, jobs_per_xcd, run_len, runs_cap, runs_rem)


@dataclass(frozen=True)
class K16Walk:
    wg: int
    job_begin: int
    job_end: int
    job_step: int
    steps: tuple        # per iteration (job, hop, pair): what the loop body sees in (job, f0 = hop_c, pair = pair_c); mono: (job, 0, 0)


def k16_walk(L: K16Launch, block: int, carry: bool = True, skip_last_step: bool = False) -> K16Walk:
    """the kernel's walk for blockIdx.x = block, variable by variable.  carry=False is the broken model of the check of the checker
    (`if (pair_c >= p.pairs) { pair_c -= p.pairs; hop_c += 1; }` dropped); skip_last_step models the omit-only variant library."""
    nx, grid, pairs = L.xcds, L.blocks, L.pairs
    xcd, local = block % nx, block // nx
    wg = xcd * (grid // nx) + local
    job_step = 1 if L.slide else grid // nx
    if L.slide:
        job_begin = (wg // pairs) * L.run_len
        job_end = min(job_begin + L.run_len, L.n_frames)
    else:
        job_begin = xcd * L.jobs_per_xcd + local
        job_end = min((xcd + 1) * L.jobs_per_xcd, L.n_jobs)
    hop_c = 0 if L.mono else job_begin if L.slide else job_begin // pairs
    pair_c = 0 if L.mono else wg % pairs if L.slide else job_begin - hop_c * pairs
    step_hops = 0 if L.mono else 1 if L.slide else job_step // pairs
    step_pairs = 0 if (L.mono or L.slide) else job_step - step_hops * pairs
    steps, job = [], job_begin
    while job < job_end:
        more = job + job_step < job_end
        if not (skip_last_step and not more and job != job_begin):
            steps.append((job, hop_c, pair_c))
        if not L.mono and more:       # the next job's (hop, pair)
            pair_c += step_pairs
            hop_c += step_hops
            if carry and pair_c >= pairs:
                pair_c -= pairs
                hop_c += 1
        job += job_step
    return K16Walk(wg, job_begin, job_end, job_step, tuple(steps))


def k16_problems(L: K16Launch, carry: bool = True) -> list:
    """every way the walk of a launch misses `each row (frame, pair) exactly once, every index in range, (hop, pair) = divmod(job, pairs)`
    (mono: the rows are the frames of its jobs, (frame, 0))"""
    bad, seen, wgs = [], {}, set()
    width = 1 if L.mono else L.pairs
    for b in range(L.blocks):
        w = k16_walk(L, b, carry)
        wgs.add(w.wg)
        for job, hop, pair in w.steps:
            if L.mono or not L.slide:
                if not 0 <= job < L.n_jobs:
                    bad.append(("job out of range", b, job))
                if not L.mono and (hop, pair) != divmod(job, L.pairs):
                    bad.append(("(hop, pair) is not divmod(job, pairs)", b, job, hop, pair))
            elif not (0 <= job < L.n_frames and hop == job and pair == w.wg % L.pairs):
                bad.append(("slide: hop or pair", b, job, hop, pair))
            rows = [(f, 0) for f in paired_frames_of(job, L.pair_base, L.first_frame, L.n_frames)] if L.mono else [(hop, pair)]
            for row in rows:
                if 0 <= row[0] < L.n_frames and 0 <= row[1] < width:
                    seen[row] = seen.get(row, 0) + 1
                else:
                    bad.append(("row out of range", b, row))
    if wgs != set(range(L.blocks)):
        bad.append(("wg is not a permutation of the grid",))
    if len(seen) != L.n_frames * width or any(v != 1 for v in seen.values()):
        bad.append(("not exactly once", len(seen), L.n_frames * width, sum(v != 1 for v in seen.values())))
    return bad


# ---- the two-pass pixel kernel ------------------------------------------------------------------------------------------------------------
def pixel_blocks(n_cu: int, per_cu: int, n_columns: int) -> int:
    return min(n_cu * min(per_cu, 8), n_columns)


def pixel_walk(blocks: int, block: int, n_columns: int):
    """(columns written, columns requested) of workgroup `block`, in the kernel's order: the prologue requests col and col + grid, the loop
    body col + 2 grid, each behind its own bound check"""
    cols, req = [], []
    col = block
    if col < n_columns:
        req.append(col)
        if col + blocks < n_columns:
            req.append(col + blocks)
    while col < n_columns:
        cols.append(col)
        if col + blocks < n_columns and col + 2 * blocks < n_columns:
            req.append(col + 2 * blocks)
        col += blocks
    return cols, req


def pixel_problems(blocks: int, n_columns: int) -> list:
    bad, seen = [], {}
    for b in range(blocks):
        cols, req = pixel_walk(blocks, b, n_columns)
        if req != cols:
            bad.append(("the requested columns are not the written ones, in order", b))
        if any(not 0 <= c < n_columns for c in cols + req):
            bad.append(("column out of range", b))
        for c in cols:
            seen[c] = seen.get(c, 0) + 1
    if len(seen) != n_columns or any(v != 1 for v in seen.values()):
        bad.append(("not exactly once", len(seen), n_columns))
    return bad


# ---- the inverse ---------------------------------------------------------------------------------------------------------------------------
def istft_split(n_cu: int, per_cu: int, pairs: int, W: int, H: int, s0: int, s1: int):
    """(b0, b_end, kw, run, groups) of launch_istft for samples [s0, s1)"""
    b0, b_end = s0 // H, (s1 - 1) // H + 1
    n_blocks, kw = b_end - b0, (W - 1) // H
    groups = max(1, n_cu * per_cu // pairs)
    run = max(ceil_div(n_blocks, groups), kw + 1)
    return b0, b_end, kw, run, ceil_div(n_blocks, run)


def istft_walk(b0, b_end, kw, run, groups) -> list:
    """per group, (blocks emitted, first block transformed): ta = b0 + g run, the warm-up from max(ta - kw, 0)"""
    out = []
    for g in range(groups):
        ta = b0 + g * run
        if ta >= b_end:
            out.append(([], None))
            continue
        out.append((list(range(ta, min(ta + run, b_end))), max(ta - kw, 0)))
    return out


def istft_problems(split) -> list:
    b0, b_end, kw, run, groups = split
    seen = [b for emitted, _ in istft_walk(*split) for b in emitted]
    return [] if seen == list(range(b0, b_end)) else [("not exactly once, in order", len(seen), b_end - b0)]


# ---- the table of tests/test_gpu_cu_counts.py ---------------------------------------------------------------------------------------------
K16_CH6_H512 = es.Route("k16_ch6_h512", 8192, 512, 6, (), kernel=10, floor=FLOOR_K16, structure=("k16",))
K16_CH6_H1024 = es.Route("k16_ch6_h1024", 8192, 1024, 6, (), kernel=10, floor=FLOOR_K16, structure=("k16",))
EXTRA_ROUTES = {r.name: r for r in (K16_CH6_H512, K16_CH6_H1024)}


@dataclass(frozen=True)
class Case:
    name: str           # the id of the GPU test case
    route: str          # a row of edge_signals.ROUTES or EXTRA_ROUTES
    kind: str           # "forward": the batch entry points from PCM; "pixel": two-kernel pixel contexts; "inverse": sgx_istft_batch
    frames: int
    first: int          # the odd first_frame of the sub-range (forward, pixel) / the first sample of the sub-range (inverse)
    frames_32: int = 0  # frames at limit 32 where that differs (0: the same)


def route_of(case: Case) -> es.Route:
    return EXTRA_ROUTES.get(case.route) or es.ROUTE[case.route]


# W 2048 / W 2400: 75 frames -- at limit 1 four (three) workgroups of 19 (25) jobs, the last run ragged; mono: an odd count, so that the
# last job of the last run holds one frame.  W 8192: hop counts that give n_jobs >= 8 * blocks at limits 8 and 16 (xcds = 8, more than
# one job per workgroup), a ragged last XCD, and with pairs = 3 a job_step that is no multiple of the pairs.
TABLE = [Case(n, n, "forward", 75, 3) for n in ("k1r_h256", "k1r_h100", "k1r_h256_align4", "k1_lr_h256", "k1_lr_h58", "k1_complex_mono",
                                                "k1_paired_mono", "k1_ch4", "k1_ch8", "k48_lr", "k48_paired_mono")]
TABLE += [
    Case("k16_lr_h512", "k16_lr_h512", "forward", 67, 3),
    # limit 32: n_jobs >= 8 * 32 on the two-channel row, and no more than the 256 CUs of the device: the limit-0 reference keeps one job
    # per workgroup, which the omit-only variant libraries leave alone (references_have_one_job)
    Case("k16_lr_h300", "k16_lr_h300", "forward", 131, 5, frames_32=256),
    Case("k16_ch8_h512", "k16_ch8_h512", "forward", 33, 3),
    Case("k16_ch8_h300", "k16_ch8_h300", "forward", 33, 3),
    Case("k16_mono_h512", "k16_mono_h512", "forward", 67, 3),
    Case("k16_ch6_h512", "k16_ch6_h512", "forward", 43, 3),
    Case("k16_ch6_h1024", "k16_ch6_h1024", "forward", 43, 3),
    Case("pixel_w2048_two_kernel", "k1_lr_h256", "pixel", 75, 3),
    Case("pixel_w735_runtime", "mixed_w735_runtime_lr", "pixel", 75, 3),
    Case("pixel_w256_generic", "generic_w256_lr", "pixel", 75, 3),
    Case("pixel_w2400", "k48_lr", "pixel", 75, 3),
    Case("pixel_w4096", "mixed_w4096_lr", "pixel", 75, 3),
    Case("pixel_w5000_real", "mixed_w5000_runtime_real", "pixel", 75, 3),
    Case("pixel_w8192", "k16_lr_h300", "pixel", 75, 3),
    Case("pixel_w10290_column", "large_w10290_mono", "pixel", 41, 3),
    Case("inverse_k1_lr_h256", "k1_lr_h256", "inverse", 75, 2048 + 257),
    Case("inverse_k48_lr", "k48_lr", "inverse", 75, 2400 + 95),
    Case("inverse_k16_ch8_h512", "k16_ch8_h512", "inverse", 33, 8192 + 513),
    Case("inverse_chirpz_w1102_lr", "chirpz_w1102_lr", "inverse", 75, 1102 + 277),
]
CASE = {c.name: c for c in TABLE}
assert len(CASE) == len(TABLE)

REQUIRED_BRANCHES = (
    "k16: xcds == 8, more than one job per workgroup", "k16: xcds == 1, more than one job per workgroup",
    "k16: job_step < pairs", "k16: job_step % pairs != 0", "k16: job_step % pairs == 0 (pairs > 1)",
    "k16: H == 512, slide", "k16: H == 512, no slide (pairs > n_cu)",
    "k16: runs = n_cu / pairs without remainder", "k16: runs = n_cu / pairs with remainder",
    "ragged last run", "a workgroup with exactly one job", "a workgroup with no job",
    "run_split: prologue, steady state and last job in one run", "run_split: a last job without its second frame",
    "pixel: every workgroup walks at least 3 columns", "inverse: a run no longer than its warm-up")


# The classes of launch_render the pixel cases take, as tests/pixel_plans.py restates them with the seeded 256-entry palette the cases use:
# (render_class, workgroups per CU that LDS and threads allow).  One case per class that pixel_plans.blocks_launched distinguishes among the
# routes' windows: every block size of the two-pass kernel, images of one, two, four and eight workgroups per CU (W 8192: 126 KB, above the
# 64 KB that need the opt-in), and the per-column kernel, whose grid does not follow the count (its helper passes magnitude_in and
# render_bands do).  tests/test_cu_counts.py holds this table to pixel_plans.
PIXEL_CLASSES = {
    "pixel_w2048_two_kernel": (("two_pass", 256, 8, 12), 4), "pixel_w735_runtime": (("two_pass", 256, 8, 12), 8),
    "pixel_w256_generic": (("two_pass", 256, 8, 12), 8), "pixel_w2400": (("two_pass", 256, 10, 12), 4),
    "pixel_w4096": (("two_pass", 512, 8, 0), 2), "pixel_w5000_real": (("two_pass", 512, 16, 0), 2),
    "pixel_w8192": (("two_pass", 1024, 8, 0), 1), "pixel_w10290_column": (("column", True, True), 8)}


def frames_at(case: Case, limit: int) -> int:
    return case.frames_32 if limit == 32 and case.frames_32 else case.frames


def run_split_per_cu(r: es.Route):
    """workgroups per CU of the run_split launchers, None for the routes that do not come through run_split"""
    return 4 if r.kernel == 2 else 3 if r.kernel == 9 and r.channels <= 2 and (r.channels == 2 or r.paired) else None


def forward_calls(case: Case, limit: int) -> list:
    """[(first_frame, n_frames)]: the whole range, and the sub-range from the case's odd first_frame"""
    F = frames_at(case, limit)
    return [(0, F), (case.first, F - case.first)]


def forward_split(r: es.Route, n_cu: int, first: int, n: int):
    """("run_split", per, blocks, frames of every job) or ("k16", K16Launch) for the transform launch of frames [first, first + n)"""
    per_cu = run_split_per_cu(r)
    if per_cu is not None:
        if r.paired:
            base, n_jobs = paired_jobs(first, n)
            frames = [paired_frames_of(j, base, first, n) for j in range(n_jobs)]
        elif r.kernel == 2 and r.channels == 1 and "complex_mono" not in r.flags:   # stft4096_real.hip, at any alignment of the stream
            n_jobs = (n + 1) // 2
            frames = [real_frames_of(j, n) for j in range(n_jobs)]
        else:
            n_jobs, frames = n, [[f] for f in range(n)]
        per, blocks = run_split(n_cu, n_jobs, per_cu)
        return "run_split", per, blocks, frames
    assert r.kernel == 10
    return "k16", k16_launch(n_cu, n, r.pairs, r.H, r.paired, first)


def branches(case: Case, limit: int, device_cu: int) -> set:
    """the names of REQUIRED_BRANCHES that (case, limit) takes, over both of its calls"""
    r, n_cu, out = route_of(case), limit_value(limit, device_cu), set()
    F = frames_at(case, limit)
    if case.kind == "pixel":
        if F >= 3 * n_cu * 8:     # (the launcher's own cap of 8 workgroups per CU: whatever the occupancy API answers)
            out.add("pixel: every workgroup walks at least 3 columns")
        return out
    if case.kind == "inverse":
        N = (F - 1) * r.H + r.W
        for s0, s1 in ((0, N), (case.first, N)):
            _, _, kw, run, _ = istft_split(n_cu, 1, r.pairs, r.W, r.H, s0, s1)   # (one workgroup per CU: the longest run any occupancy gives)
            if run == kw + 1:
                out.add("inverse: a run no longer than its warm-up")
        return out
    for first, n in forward_calls(case, limit):
        split = forward_split(r, n_cu, first, n)
        if split[0] == "run_split":
            _, per, blocks, frames = split
            walk = run_walk(per, blocks, len(frames))
            lens = [len(w) for w in walk]
            if lens[-1] < per:
                out.add("ragged last run")
            if 1 in lens:
                out.add("a workgroup with exactly one job")
            if max(lens) >= 3:
                out.add("run_split: prologue, steady state and last job in one run")
            if any(len(frames[w[-1]]) == 1 and len(w) >= 2 for w in walk if w) and any(len(f) == 2 for f in frames):
                out.add("run_split: a last job without its second frame")
            continue
        L = split[1]
        lens = [len(k16_walk(L, b).steps) for b in range(L.blocks)]
        many = max(lens) > 1
        if 1 in lens:
            out.add("a workgroup with exactly one job")
        if 0 in lens:
            out.add("a workgroup with no job")
        if r.H == 512 and not L.mono:
            out.add("k16: H == 512, slide" if L.slide else "k16: H == 512, no slide (pairs > n_cu)")
        if L.slide:
            if L.runs_cap <= L.n_frames:      # (else the frames, not the CUs, bound the runs)
                out.add("k16: runs = n_cu / pairs " + ("with remainder" if L.runs_rem else "without remainder"))
            if min(lens) < max(lens):
                out.add("ragged last run")
            continue
        if many:
            out.add("k16: xcds == %d, more than one job per workgroup" % L.xcds)
        if many and not L.mono:
            step = L.blocks // L.xcds
            if step < L.pairs:
                out.add("k16: job_step < pairs")
            if L.pairs > 1:
                out.add("k16: job_step % pairs != 0" if step % L.pairs else "k16: job_step % pairs == 0 (pairs > 1)")
    return out


def bank_kinds(r: es.Route) -> tuple:
    """the filterbank calls a forward case runs besides its other entry points: on the 4096-point kernels sgx_fbank_batch and, with an
    (l, r) pair, sgx_fbank_cross_batch.  Their fused modes (bounds_arena.fbank_fused) are instantiations of the same persistent kernels
    behind the same launcher: forward_split is their split as well, and on the workspace route (frame pairs, the complex mono transform)
    it is the split of the rows they read."""
    if r.kernel != 2:
        return ()
    return ("fbank", "fbank_cross") if r.channels >= 2 else ("fbank",)


def welch_kinds(r: es.Route) -> tuple:
    """the Welch calls a forward case runs besides its other entry points: sgx_psd_batch at group 3 on every case and, with an (l, r)
    pair, sgx_csd_batch.  No context runs them fused: they are always on the workspace route, so the split under test is that of the
    rows (magnitudes, complex) the call reads -- forward_split of the same frames -- and the two kernels of sgx_psd.hip behind it take
    nothing from the compute-unit count."""
    return ("psd_3", "csd_3") if r.channels >= 2 else ("psd_3",)


LAST_JOB_ONE_FRAME = "run_split: a last job without its second frame"


def bank_cases_with_a_last_job_of_one_frame(device_cu: int) -> list:
    """[(case name, limit)] at which a FUSED bank call meets a run whose last job lacks its second frame: the real-input kernel holds two
    frames' magnitudes in one column there, and its filter pass must write one frame's sums only"""
    return [(c.name, limit) for c in TABLE if c.kind == "forward" and bank_kinds(route_of(c)) and ba.fbank_fused(route_of(c))
            for limit in LIMITS if LAST_JOB_ONE_FRAME in branches(c, limit, device_cu)]


def more_than_one_job(case: Case, limit: int, device_cu: int, family: str) -> bool:
    """does a workgroup of the `family` ("run_split" / "k16") launch of (case, limit) run more than one job, in either of its calls --
    the cases an omit-only variant library of that family must fail"""
    if case.kind != "forward":
        return False
    r, n_cu = route_of(case), limit_value(limit, device_cu)
    for first, n in forward_calls(case, limit):
        split = forward_split(r, n_cu, first, n)
        if split[0] != family:
            continue
        if family == "run_split":
            if split[1] > 1 and len(split[3]) > 1:
                return True
        elif max(len(k16_walk(split[1], b).steps) for b in range(split[1].blocks)) > 1:
            return True
    return False


def references_have_one_job(device_cu: int, family: str) -> bool:
    """at the device's own count, does every call of every forward case -- at each of its frame counts -- give no workgroup of `family`
    more than one job?  Then an omit-only variant library of that family computes every limit-0 reference in full."""
    for case in TABLE:
        if case.kind != "forward":
            continue
        r = route_of(case)
        for limit in LIMITS:     # (the calls a limit makes, run at the device's count: that is how its reference is made)
            for first, n in forward_calls(case, limit):
                split = forward_split(r, device_cu, first, n)
                if split[0] != family:
                    continue
                if family == "run_split" and split[1] > 1:
                    return False
                if family == "k16" and max(len(k16_walk(split[1], b).steps) for b in range(split[1].blocks)) > 1:
                    return False
    return True


def peak_fpj(r: es.Route) -> int:
    """frames per job of the fused peak route: 2 on the real-input kernel, 1 on the (l, r) kernel"""
    return 2 if r.kernel == 2 and r.channels == 1 and not r.flags else 1


def peak_run_group(r: es.Route, n: int, n_cu: int) -> int:
    """a peak group equal to one run of the limit in force on the fused peak route (bounds_arena.fused_peak_run)"""
    return ba.fused_peak_run(n, n, n_cu, peak_fpj(r))
