"""tests/quantile_reference.py (the numpy restatement of sgx_quantile_batch's definition in include/sgx.h) against a plain Python loop,
bit for bit, and against results known by hand: the rank table, the total order of the special values, ties, a short last column, and
the range arithmetic of the host dispatch."""
import math

import numpy as np
import pytest

import quantile_reference as ref

LENGTHS = (1, 2, 3, 32, 33, 255, 256, 257)
Q5 = (0.0, 0.1, 0.5, 0.9, 1.0)


def py_key(u):
    return u ^ (0xFFFFFFFF if u >> 31 else 0x80000000)


def py_quantiles(rows, group, q):
    """the definition, word by word: sorted() on integer keys"""
    flat = rows.reshape(rows.shape[0], -1).view(np.uint32)
    out = []
    for f, n in ref.columns(rows.shape[0], group):
        col = []
        for qi in q:
            k = int(math.floor(qi * float(n - 1) + 0.5))
            row = []
            for e in range(flat.shape[1]):
                keys = sorted(py_key(int(flat[t, e])) for t in range(f, f + n))
                w = keys[k]
                row.append(w ^ (0x80000000 if w >> 31 else 0xFFFFFFFF))
            col.append(row)
        out.append(col)
    return np.array(out, dtype=np.uint32)


def wild(rng, shape):
    """random words of every class: both signs, zeros, infinities, NaNs of both signs, ties"""
    v = rng.standard_normal(shape).astype(np.float32)
    pick = rng.integers(0, 12, shape)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32)
    v = np.where(pick < 7, v, special[pick % 7])
    w = v.view(np.uint32).copy()
    w[pick == 11] = 0xFFC00001                                                    # a negative NaN
    return w.view(np.float32)


@pytest.mark.parametrize("n", LENGTHS)
def test_against_a_python_loop(n):
    rng = np.random.default_rng(n)
    for rows in (rng.random((n, 2, 3, 2), dtype=np.float32), wild(rng, (n, 7))):
        for q in (Q5, (0.5,), tuple(np.linspace(1.0, 0.0, 16)), (0.25, 0.25, 0.75)):
            for group in sorted({1, 2, n, n + 10, max(n // 2, 1), 5}):
                got = ref.quantiles(rows, group, q)
                want = py_quantiles(rows, group, q)
                assert got.shape == (len(ref.columns(n, group)), len(q)) + rows.shape[1:]
                assert np.array_equal(got.reshape(want.shape).view(np.uint32), want), (n, group, q)


def test_rank_table():
    table = {2: (0, 0, 1, 1, 1), 3: (0, 0, 1, 2, 2), 32: (0, 3, 16, 28, 31), 33: (0, 3, 16, 29, 32), 255: (0, 25, 127, 229, 254),
             256: (0, 26, 128, 230, 255), 257: (0, 26, 128, 230, 256)}
    for n, ranks in table.items():
        assert tuple(ref.rank(q, n) for q in Q5) == ranks, n
    assert ref.rank(0.5, 2) == 1 and ref.rank(0.0, 1) == ref.rank(1.0, 1) == 0   # a half goes up; a column of one frame
    for n in LENGTHS:
        assert ref.rank(0.0, n) == 0 and ref.rank(1.0, n) == n - 1


def test_group_one_reproduces_the_rows():
    rng = np.random.default_rng(1)
    rows = wild(rng, (9, 5, 2))
    got = ref.quantiles(rows, 1, Q5)
    for i in range(len(Q5)):
        assert np.array_equal(got[:, i].view(np.uint32), rows.view(np.uint32))


@pytest.mark.parametrize("n", LENGTHS)
def test_ends_are_min_and_max(n):
    rows = np.random.default_rng(n + 100).random((n, 11), dtype=np.float32)
    rows[rows < 0.1] = 0.0
    got = ref.quantiles(rows, n, (0.0, 1.0))
    assert np.array_equal(got[0, 0].view(np.uint32), rows.min(0).view(np.uint32))
    assert np.array_equal(got[0, 1].view(np.uint32), rows.max(0).view(np.uint32))
    assert np.array_equal(ref.quantiles(rows, n, Q5).view(np.uint32), np.sort(rows, 0)[[ref.rank(q, n) for q in Q5]][None].view(np.uint32))


def test_ties_and_constant_columns():
    const = np.full((33, 4), 0.25, dtype=np.float32)
    assert (ref.quantiles(const, 33, Q5) == 0.25).all()
    for low in range(0, 34):                                                      # `low` frames hold 1, the others 2: the tie count meets every rank
        rows = np.where(np.arange(33)[:, None] % 33 < low, 1.0, 2.0).astype(np.float32)
        rows = rows[np.random.default_rng(low).permutation(33)]
        got = ref.quantiles(rows, 33, Q5)[0, :, 0]
        assert got.tolist() == [1.0 if ref.rank(q, 33) < low else 2.0 for q in Q5], low


def test_total_order_of_the_special_values():
    words = np.array([0xFFC00000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00000], dtype=np.uint32)
    # -NaN, -inf, -1, -0, +0, 1, +inf, +NaN
    keys = ref.key(words)
    assert (np.diff(keys.astype(np.int64)) > 0).all()
    assert np.array_equal(ref.unkey(keys), words)
    rng = np.random.default_rng(8)
    rows = words[rng.permutation(8)].view(np.float32).reshape(8, 1)
    got = ref.quantiles(rows, 8, tuple(i / 7.0 for i in range(8)))
    assert np.array_equal(got.view(np.uint32).reshape(-1), words)
    every = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(ref.unkey(ref.key(every)), every)
    # on rows >= +0 with NaN the order is np.sort's
    mags = rng.random((40, 6), dtype=np.float32)
    mags[3, 2] = mags[17, 2] = np.nan
    mags[5, 1] = np.inf
    assert np.array_equal(ref.quantiles(mags, 40, tuple(i / 39.0 for i in (0, 7, 20, 38, 39))).view(np.uint32)[0],
                          np.sort(mags, 0)[[0, 7, 20, 38, 39]].view(np.uint32))


def test_a_short_last_column():
    rows = np.random.default_rng(3).random((70, 3), dtype=np.float32)
    got = ref.quantiles(rows, 32, Q5)
    assert got.shape == (3, 5, 3) and ref.columns(70, 32) == [(0, 32), (32, 32), (64, 6)]
    assert np.array_equal(got[2], ref.quantiles(rows[64:], 6, Q5)[0])
    assert np.array_equal(got[2, 2], np.sort(rows[64:], 0)[3])                    # floor(0.5 * 5 + 0.5) = 3
    assert np.array_equal(ref.quantiles(rows, ref.SIZE_MAX, Q5), ref.quantiles(rows, 70, Q5))
    assert ref.columns(0, 5) == []


def test_arguments():
    assert ref.valid_q((0.0, 1.0, 0.5, 0.5)) and ref.valid_q((0.5,) * 16)
    for bad in ((), (0.5,) * 17, (-0.1,), (1.0000001,), (float("nan"),), (0.5, float("nan"))):
        assert not ref.valid_q(bad), bad


def test_range_arithmetic():
    row = 2047 * 2 * 4
    assert ref.cap(row) == 12294 and ref.cap(4 * row) == 3073 and ref.cap(16384 * row) == 1 and ref.cap(ref.WORKSPACE_BYTES) == 1
    for n, group, rb in ((4000, 33, 4 * row), (3073, 3073, 4 * row), (5000, 1, 4 * row), (100, 1000, row), (7, 1, 16384 * row), (12294, ref.SIZE_MAX, row)):
        ranges = ref.plan(n, group, rb)
        g, c = min(group, n), ref.cap(rb)
        nxt = 0
        for f, m, col in ranges:
            assert f == nxt and 1 <= m <= c and f % g == 0 and col == f // g      # in order, within the workspace, on a column boundary
            assert m % g == 0 or f + m == n                                       # whole columns; only the call's last column is short
            nxt = f + m
        assert nxt == n
        assert all(m == c // g * g for _, m, _ in ranges[:-1])
    assert len(ref.plan(4000, 33, 4 * row)) == 2 and ref.plan(4000, 33, 4 * row)[0][1] == 93 * 33
    # the refusal: a column longer than the cap, by group or by the call's own length
    assert ref.plan(3074, 3074, 4 * row) is None and ref.plan(3074, ref.SIZE_MAX, 4 * row) is None
    assert ref.plan(3073, 3074, 4 * row) is not None and ref.plan(2, 2, 16384 * row) is None and ref.plan(2, 1, 16384 * row) is not None
