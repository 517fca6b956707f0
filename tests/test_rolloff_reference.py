"""tests/rolloff_reference.py, the numpy restatement of sgx_rolloff_batch / sgx_rolloff_mags (include/sgx.h), without a GPU: bit for bit
against a Python loop of np.float32 scalars, monotone, right on rows known by hand, within the arithmetic bound of float64, and in
agreement with what a caller would write instead wherever float64 decides the crossing."""
import math

import numpy as np
import pytest

import rolloff_reference as ref

LENGTHS = (1, 3, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049)
U = 2.0 ** -24
EIGHT = (0.005, 0.05, 0.25, 0.5, 0.75, 0.85, 0.95, 0.995)


def np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def one(m, power, p):
    """rolloff() of a single row on both sides -> [n_p][4]"""
    rows = np.stack([m, m], -1).astype(np.float32)
    got = ref.rolloff(rows, power, p)
    assert np.array_equal(np_bits(got[0]), np_bits(got[1]))
    return got[0]


@pytest.mark.parametrize("M", LENGTHS)
def test_bit_for_bit_against_the_loop(M):
    rng = np.random.default_rng(1000 + M)
    crafted = ref.crafted_rows(M, rng)
    names = sorted(crafted)
    if M > 100:                                                  # (the loop is slow: the rows a long row can go wrong on)
        names = ["noise", "noise_wide", "tile_ends", "segment_ends", "nan_in_the_middle", "huge_first"]
    rows = np.stack([np.stack([crafted[n], crafted[names[(i + 1) % len(names)]]], -1) for i, n in enumerate(names)])
    p = (0.85, 0.05, 0.85, 2.0 ** -20, 1.0)
    for power in (1, 2):
        c = ref.cumulative(rows, power)
        r = ref.rolloff(rows, power, p)
        assert c.shape == rows.shape and c.dtype == np.float32 and r.shape == (len(names), 2, len(p), 4) and r.dtype == np.float32
        for i in range(len(names)):
            for s in range(2):
                assert np.array_equal(np_bits(c[i, :, s]), np_bits(ref.cumulative_loop(rows[i, :, s], power))), (names[i], s, power)
                assert np.array_equal(np_bits(r[i, s]), np_bits(ref.rolloff_loop(rows[i, :, s], power, p))), (names[i], s, power)


@pytest.mark.parametrize("M", LENGTHS + (8191,))
def test_cumulative_never_decreases(M):
    rng = np.random.default_rng(2000 + M)
    crafted = ref.crafted_rows(M, rng)
    names = [n for n in sorted(crafted) if n != "nan_in_the_middle"]
    rows = np.stack([np.stack([crafted[n], crafted[n][::-1]], -1) for n in names])
    for power in (1, 2):
        c = ref.cumulative(rows, power)
        assert (c[:, 1:] >= c[:, :-1]).all()
        assert (c[:, 0] >= 0).all()


def test_rows_known_by_hand():
    M = 2048
    ones = np.ones(M, np.float32)
    for power in (1, 2):
        r = one(ones, power, (0.5,))
        assert r.tolist() == [[1024.0, 1023.0, 1024.0, 2048.0]]  # thr = 1024 = c[1023] exactly: >= decides the tie
        assert ref.cumulative(np.stack([ones, ones], -1), power)[1023, 0] == 1024.0
    for M in (33, 2047, 2049):
        for j in sorted({0, M - 1, 31, 32}):
            m = np.zeros(M, np.float32)
            m[j] = 3.0
            for power, t in ((1, 3.0), (2, 9.0)):
                r = one(m, power, (2.0 ** -20, 0.5, 1.0))
                assert (r == np.array([j + 1, 0.0, t, t], np.float32)).all(), (M, j, power)
        for power in (1, 2):
            r = one(np.zeros(M, np.float32), power, (0.5, 1.0))
            assert np.array_equal(np_bits(r), np_bits(np.zeros((2, 4))))                         # (0, 0, 0, +0)
            m = np.random.default_rng(M).random(M).astype(np.float32)
            m[M // 2] = np.nan
            r = one(m, power, (0.5, 1.0))
            assert (r[:, :3] == 0).all() and np.isnan(r[:, 3]).all()
            m = np.ones(M, np.float32)
            m[0] = 1e30
            r = one(m, power, EIGHT)
            assert (r[:, 0] == 1).all() and (r[:, 1] == 0).all() and (r[:, 2] == (np.float32(1e30) if power == 1 else np.inf)).all()


@pytest.mark.parametrize("M", LENGTHS + (8191,))
def test_share_one_always_finds_a_bin(M):
    rng = np.random.default_rng(3000 + M)
    rows = (rng.random((16, M, 2)) * np.exp(8.0 * rng.random((16, M, 2)))).astype(np.float32)
    if M > 1:
        rows[3, M // 2:] = 0                                     # the total is reached before the row ends: the first j, not the last
    for power in (1, 2):
        c = ref.cumulative(rows, power)
        r = ref.rolloff(rows, power, (1.0,))
        assert (r[..., 0, 0] >= 1).all() and (r[..., 0, 0] <= M).all()
        assert np.array_equal(np_bits(r[..., 0, 2]), np_bits(r[..., 0, 3])) and np.array_equal(np_bits(r[..., 0, 3]), np_bits(c[:, -1, :]))
        assert (r[..., 0, 1] < r[..., 0, 2]).all()
        assert M == 1 or (r[3, :, 0, 0] <= M // 2).all()


def bound(M):
    """include/sgx.h, the issue's count of roundings: one for the square plus 31 for the segment chain, one per segment total in the
    offset chain, the final add plus slack; times 1.01 for second-order terms"""
    return (32 + math.ceil(M / 32) + 2) * U * 1.01


@pytest.mark.parametrize("M", LENGTHS + (8191,))
def test_arithmetic_bound_against_float64(M):
    rng = np.random.default_rng(4000 + M)
    rows = np.concatenate([rng.random((8, M, 2)), rng.random((8, M, 2)) * np.exp(8.0 * rng.random((8, M, 2))),
                           np.ones((1, M, 2))]).astype(np.float32)
    for power in (1, 2):
        c = ref.cumulative(rows, power).astype(np.float64)
        c64 = np.cumsum(rows.astype(np.float64) ** power, axis=-2)
        t64 = c64[:, -1:, :]
        worst = float((np.abs(c - c64) / (bound(M) * t64)).max())
        print(f"M {M} power {power}: worst |c - C64| / (bound * T64) = {worst:.4f} (bound {bound(M) / U:.1f} * 2^-24)")
        assert worst <= 1.0


@pytest.mark.parametrize("M", (33, 2047, 2049, 8191))
def test_against_a_plain_float32_cumsum_and_searchsorted(M):
    """What a caller would write: np.cumsum of the whole row in float32 and np.searchsorted.  That chain has M - 1 roundings, one per
    element, so its own error is up to (M + 1) * 2^-24 of the total, which also covers the definition's.  Both thresholds carry the
    error of their total and one rounding.  Where the float64 crossing clears p * T64 on both sides by three times that, both must name
    the float64 bin.  The rows are a few peaks on a low floor, so that most crossings lie inside a peak and are that clear."""
    rng = np.random.default_rng(5000 + M)
    rows = 1e-6 * rng.random((32, M, 2))
    for f in range(32):
        for s in range(2):
            at = rng.choice(M, size=min(48, M // 2), replace=False)
            rows[f, at, s] = 0.25 + rng.random(at.shape[0])
    rows = rows.astype(np.float32)
    delta = 3.0 * (M + 1) * U * 1.01
    decided = total = 0
    for power in (1, 2):
        got = ref.rolloff(rows, power, EIGHT)
        x = rows * rows if power == 2 else rows
        plain = np.cumsum(x, axis=-2, dtype=np.float32)
        c64 = np.cumsum(rows.astype(np.float64) ** power, axis=-2)
        for f in range(rows.shape[0]):
            for s in range(2):
                for i, p in enumerate(EIGHT):
                    t64 = c64[f, -1, s]
                    j64 = int(np.searchsorted(c64[f, :, s], p * t64, side="left"))
                    jp = int(np.searchsorted(plain[f, :, s], np.float32(p) * plain[f, -1, s], side="left"))
                    total += 1
                    clear = c64[f, j64, s] - p * t64 > delta * t64 and (j64 == 0 or p * t64 - c64[f, j64 - 1, s] > delta * t64)
                    if clear:
                        decided += 1
                        assert got[f, s, i, 0] == j64 + 1 == jp + 1, (M, power, f, s, p)
    print(f"M {M}: float64 decides {decided} of {total} crossings by more than {delta / U:.0f} * 2^-24 of the total")
    assert decided >= total // 2
