"""The case table, the labelling and the streams of tests/channel_counts.py, and the two offset bounds sgx_create's cap of 32 768 channels
rests on (no GPU).  tests/test_gpu_channel_counts.py then holds every family to these streams at 6, 12, 64 and 32 768 channels."""
import numpy as np
import pytest

import bounds_arena as ba
import channel_counts as cn
import edge_signals as es
import oracle
from conftest import FLOOR_K16, FLOOR_WIDE, mags_error


def test_the_table_holds_every_family_at_every_count():
    names = [c.name for c in cn.ALL]
    assert len(set(names)) == len(names)
    by = {(c.family, c.channels) for c in cn.TABLE}
    assert by == {(f, n) for f in cn.SHAPES for n in (6, 12, 64)}
    assert {c.family for c in cn.CAP_ROWS} == {f for f, s in cn.SHAPES.items() if s[8] is not None}
    assert {c.family: (c.W, c.H, c.frames) for c in cn.CAP_ROWS} == {
        "generic_w64": (64, 16, 2), "bluestein_w23": (23, 5, 2), "mixed_w735_runtime": (735, 200, 2), "k1_h256": (2048, 256, 1),
        "k16_h512": (8192, 512, 1)}
    shapes = {(c.W, c.H) for c in cn.TABLE}
    assert shapes == {(2048, 256), (2048, 58), (8192, 512), (8192, 300), (2400, 93), (735, 200), (1102, 275), (23, 5), (64, 16),
                      (10290, 5148), (6001, 3003)}
    for c in cn.ALL:
        r = c.route
        assert (r.channels == cn.CAP if c.cap else r.channels in cn.COUNTS) and r.pairs == r.channels // 2
        assert c.frames == (7 if r.kernel == 11 else 9) or c.cap
        assert r.floor == (FLOOR_K16 if c.W == 8192 else FLOOR_WIDE)
        assert ("large_transforms" in r.flags) == (r.kernel == 11)
        assert c.host_bytes() <= cn.MAX_HOST_BYTES, (c.name, c.host_bytes())
        assert c.complex_and_banks == (not (c.cap and c.W in (2048, 8192)))
        # the same kernel and render_path bits as the rows of the route table with more than two channels, or with two
        twin = [e for e in es.ROUTES if (e.W, e.H, e.flags) == (r.W, r.H, r.flags) and e.channels >= 2]
        if twin:
            e = max(twin, key=lambda e: e.channels)
            if not (r.W == 2400 and e.channels == 2):     # (the 4800-point kernel serves two channels only)
                assert (e.kernel, e.bits_set, e.bits_clear) == (r.kernel, r.bits_set, r.bits_clear), (c.name, e.name)
    assert set(cn.CU_ROWS) <= set(cn.CASE) and all(cn.CASE[n].channels == 6 for n in cn.CU_ROWS)
    assert cn.cu_limits(3) == (1, 2, 3, 4, 7)
    # 6: three pairs and no multiple of 4 channels; 12: six pairs and a multiple; 64: 32 pairs
    assert [(n // 2, n % 4) for n in cn.COUNTS] == [(3, 2), (6, 0), (32, 0)]


def test_lowbias32_is_the_oracles():
    xs = np.array([0, 1, 2, 255, 256, 16383, 0x7FFFFFFF, 0xFFFFFFFF, 0x5EED0001], np.uint32)
    assert [int(v) for v in cn.lowbias32(xs)] == [int(oracle.lib().orc_lowbias32(int(x))) for x in xs]


def test_the_labelling_separates_the_index_errors_of_offset_arithmetic():
    lab = cn.labels()
    assert lab.shape == (cn.CAP // 2,) and lab.min() == 0 and lab.max() == cn.N_LABELS - 1
    counts = np.bincount(lab, minlength=cn.N_LABELS)
    assert counts.min() >= 1, "every label must be used"
    ds = cn.label_distances()
    assert set(range(1, 9)) <= set(ds) and {8192, 8191, 3 * 4096, 3, 6, 12, 15, 16} <= set(ds) and 16384 not in ds
    assert all(0 < d < cn.CAP // 2 for d in ds)
    shares = cn.labelling_shares()
    worst = max(shares, key=shares.get)
    print(f"labels: {counts.min()} .. {counts.max()} pairs per label; worst share {shares[worst]:.4%} at d = {worst}")
    assert max(shares.values()) < 0.02, (worst, shares[worst])
    # what a constant labelling, or one of period 256, would read
    assert float((np.arange(16384) % 256 == (np.arange(16384) + 256) % 256).mean()) == 1.0


def test_cap_stream_carries_the_labelled_base_pairs():
    c = cn.CASE["generic_w64_cap"]
    pcm = cn.build_stream(c)
    assert pcm.shape == (c.samples, cn.CAP) and pcm.dtype == np.float32
    base, lab = cn.base_pairs(c), cn.labels()
    for p in (0, 1, 2, 3, 4095, 4096, 8191, 8192, 16382, 16383):
        assert np.array_equal(pcm[:, 2 * p:2 * p + 2], base[lab[p]]), p
    # distinct base pairs: no two labels carry the same samples
    flat = base.reshape(cn.N_LABELS, -1)
    assert len({row.tobytes() for row in flat}) == cn.N_LABELS
    truth = cn.truth_labels(c)
    assert truth.shape == (c.frames, cn.N_LABELS, c.W - 1, 2)
    for p in (0, 5, 16383):
        assert np.array_equal(truth[1, lab[p]], es.truth_frame(es.frame_lr(cn.frame_of(c, pcm, 1), p), c.W))


@pytest.mark.parametrize("name", ["generic_w64_ch6", "k1_h58_ch12", "bluestein_w23_ch64"])
def test_stream_and_truth_against_the_oracle(name):
    c = cn.CASE[name]
    pcm = cn.build_stream(c)
    assert pcm.shape == (c.samples, c.channels) and np.isfinite(pcm).all()
    # per channel: the oracle's noise of its own seed at its pair's gain -- neighbouring pairs differ in level and in content
    rms = np.sqrt((pcm.astype(np.float64) ** 2).mean(0))
    for p in range(c.pairs):
        want = 0.25 / np.sqrt(3) * 2.0 ** -(p % 4)
        assert abs(rms[2 * p] / want - 1) < 0.2 and abs(rms[2 * p + 1] / want - 1) < 0.2, (name, p)
    assert len({pcm[:, ch].tobytes() for ch in range(c.channels)}) == c.channels
    truth = cn.truth_rows(c, pcm)
    assert truth.shape == (c.frames, c.pairs, c.W - 1, 2)
    for t, p in ((0, 0), (c.frames - 1, c.pairs - 1), (3, 1)):
        assert np.array_equal(truth[t, p], oracle.np_truth_frame(es.frame_lr(cn.frame_of(c, pcm, t), p), c.W))
    # ... and the reference's own float32 stream loop (oracle.stream_process) within the project's bound for two float32 transforms
    ref = oracle.stream_process(pcm, c.channels, c.W, c.H)
    assert ref.shape == truth.shape
    err = mags_error(ref, truth, c.route.floor)
    print(f"{name}: oracle.stream_process against the truth {err:.3f} x")
    assert err <= 2.0, (name, err)
    same = cn.identical_stream(c)
    assert same.shape == pcm.shape
    for p in range(1, c.pairs):
        assert np.array_equal(same[:, 2 * p:2 * p + 2], same[:, :2])


def test_a_swapped_pair_misses_the_truth():
    # the teeth of the streams: rows of pair p + 1 held to the truth of pair p miss by orders of magnitude, at every gain step
    c = cn.CASE["generic_w64_ch12"]
    truth = cn.truth_rows(c, cn.build_stream(c))
    for p in range(c.pairs - 1):
        assert mags_error(truth[:, p + 1], truth[:, p], c.route.floor) > 1000.0, p
    k = cn.CASE["generic_w64_cap"]
    t = cn.truth_labels(k)
    assert min(mags_error(t[:, a], t[:, b], k.route.floor) for a in range(0, 256, 17) for b in range(256) if a != b) > 1000.0


def test_the_offset_bounds_the_cap_rests_on():
    C = cn.CAP
    # stft_mixed_kernels.hpp: sample n of channel cl at the 32-bit index n * C + cl, for every W the mixed-radix kernels accept
    # (W <= 10 240: 2W up to 20 480, the largest composite length)
    assert all((W - 1) * C + C - 1 < 2 ** 32 for W in range(4, 10241))
    # stft16384_w.hip, the launcher's own inequality: lane offset 4 C tid (tid <= 511) plus row offset 2048 C a (a <= 15) plus one 8-byte
    # word, as a signed 32-bit byte offset below the descriptor's 2^31 - 1 records
    def fits(ch):
        return 4 * ch * (511 + 512 * 15) + 8 < 2 ** 31 - 1
    assert 4 * (511 + 512 * 15) == 32764
    # (the inequality alone holds up to 65 544 channels, 2^31 - 24 bytes, and fails from 65 546 on: sgx_create's cap of 32 768 lies a
    # factor of two inside it)
    assert fits(C) and fits(65544) and not fits(65546) and 65544 * 32764 + 8 == 2 ** 31 - 24
    # the last lane's word of the last pair ends exactly with a stream of 8192 samples
    assert 4 * (C - 2) + 4 * C * (511 + 512 * 15) + 8 == 8192 * C * 4


def test_device_ratio_is_conftests_mags_error():
    # the cap rows are compared on the device (16 384 rows of up to 64 KB): the same formula in torch float64
    import torch

    rng = np.random.default_rng(3)
    ref = np.abs(rng.standard_normal((2, 5, 63, 2))) * np.array([1.0, 1e-3, 1e-6, 0.1, 10.0])[None, :, None, None]
    x = (ref * (1 + 3e-6 * rng.standard_normal(ref.shape))).astype(np.float32)
    for floor in (FLOOR_WIDE, FLOOR_K16):
        per_row = cn.device_ratio(torch, torch.from_numpy(x), torch.from_numpy(ref), floor).numpy()
        assert per_row.shape == (2, 5)
        for t in range(2):
            for p in range(5):
                assert per_row[t, p] == pytest.approx(mags_error(x[t, p], ref[t, p], floor), rel=1e-12)
    from test_gpu_complex import complex_error
    cref = ref[..., 0:1] * np.exp(2j * np.pi * rng.random(ref.shape))
    cx = (cref * (1 + 3e-6 * rng.standard_normal(ref.shape))).astype(np.complex64)
    got = cn.device_complex_ratio(torch, torch.from_numpy(cx), torch.from_numpy(cref), FLOOR_WIDE).numpy()
    for t in range(2):
        for p in range(5):
            want = complex_error(cx[t, p], cref[t, p], FLOOR_WIDE, float(np.abs(cref[t, p]).max()))
            assert got[t, p] == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("W,H,channels", [(64, 16, 6), (23, 5, 1), (32, 40, 4)])
def test_inverse_ratio_is_check_definition(W, H, channels):
    import torch

    import test_gpu_istft as ti
    rng = np.random.default_rng(W)
    F = 6
    N = (F - 1) * H + W
    win = es.hann(W)
    env = np.zeros(N)
    for t in range(F):
        env[t * H:t * H + W] += win.astype(np.float64) ** 2
    ref = rng.standard_normal((N, channels)) * np.logspace(-3, 0, N)[:, None]
    ref[env == 0] = 0.0
    got = (ref * (1 + 4e-6 * rng.standard_normal(ref.shape))).astype(np.float32)
    want = ti.check_definition(got, ref, env, W, H, win)
    assert want > 0.1
    assert cn.inverse_ratio(torch, got, ref, env, W, H, win, ti.DEFINITION_TOL) == pytest.approx(want, rel=1e-12)


def test_the_welch_ranges_of_the_table():
    """what tests/test_gpu_channel_counts.py's Welch checks meet, by bounds_arena.welch_ranges (a restatement of psd_reduce): the 6-, 12-
    and 64-channel rows take every call in one range of whole columns; at 32 768 channels the workspace holds no row (W 2048, W 8192: a
    frame per piece, two rows of workspace all the same), fewer than a block of 32 and its partial (W 735, W 64) or two blocks (W 23)"""
    for c in cn.TABLE:
        for cross in (False, True):
            for group in sorted({1, 2, 4, c.frames}):
                plan = ba.welch_ranges(c.W, c.pairs, cross, c.frames, group, True)
                assert len(plan.ranges) == 1 and not plan.carried and not plan.piece and plan.cap >= 33, (c.name, cross, group)
    caps = {c.name: (ba.welch_cap(c.W, c.pairs, False), ba.welch_cap(c.W, c.pairs, True)) for c in cn.CAP_ROWS}
    assert caps == {"generic_w64_cap": (24, 12), "bluestein_w23_cap": (69, 34), "mixed_w735_runtime_cap": (2, 1), "k1_h256_cap": (0, 0),
                    "k16_h512_cap": (0, 0)}
    for c in cn.CAP_ROWS:
        assert ba.welch_row_bytes(c.W, c.pairs, False) == c.pairs * (c.W - 1) * 8
        for cross in (False, True):
            for group in (ba.WELCH_MAX, 2):
                plan = ba.welch_ranges(c.W, c.pairs, cross, c.frames, group, True)
                assert plan.workspace_rows <= max(plan.cap, 2), (c.name, cross, group)
                if plan.cap <= 2 and c.frames == 2:      # the block of two frames in two pieces, the second resumed
                    assert plan.piece == 1 and plan.resumed and [len(r.pieces) for r in plan.ranges] == [2], (c.name, cross, group)
                if plan.cap == 0:
                    assert plan.piece == 1 and plan.row_slots == 1 and plan.per == 1
    # a row larger than the whole workspace: 16 384 pairs of 2047 bins are 268 MB
    assert ba.welch_row_bytes(2048, cn.CAP // 2, False) > ba.WORKSPACE_BYTES
