"""The host reference of the Welch-averaged spectra (tests/psd_reference.py) against a straight loop, against float64 within the header's
bound, and the block / column / range arithmetic of the host dispatch -- without a GPU."""
import numpy as np
import pytest

import psd_reference as ref
from psd_reference import BLOCK, BOUND, SIZE_MAX


def wide_signed(shape, seed):
    """normal-range float32 values of either sign over 40 binary orders of magnitude"""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.uniform(-30.0, 10.0, shape))
    return (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


@pytest.mark.parametrize("n,group", [(1, 1), (31, 31), (33, 33), (70, 32), (70, 33), (100, 70), (67, 5), (40, SIZE_MAX)])
def test_numpy_chains_equal_a_python_loop(n, group):
    x = wide_signed((n, 7), n)
    x[n // 2, 3] = -0.0
    got, want = ref.welch_mean(x, group), ref.welch_mean_loop(x, group)
    assert got.shape == want.shape == (len(ref.columns_of(n, group)), 7)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_a_column_of_negative_zeros_is_plus_zero():
    x = np.full((5, 3), -0.0, np.float32)
    assert (ref.welch_mean(x, 5).view(np.uint32) == 0).all() and (ref.welch_mean_loop(x, 2).view(np.uint32) == 0).all()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 1000])
def test_bound_against_float64(n):
    """35 * 2^-24 times the mean of the absolute products: psd from wide-range magnitudes, csd from signed complex words"""
    mags = np.abs(wide_signed((n, 257, 2), 100 + n))
    got = ref.welch_mean(ref.psd_terms(mags), SIZE_MAX).astype(np.float64)
    m64 = mags.astype(np.float64) ** 2
    err, allow = np.abs(got - ref.mean64(m64, SIZE_MAX)), BOUND * ref.mean64(m64, SIZE_MAX)
    worst = float((err / allow).max())
    spec = wide_signed((n, 129, 2, 2), 200 + n)
    got = ref.welch_mean(ref.csd_terms(spec), SIZE_MAX).astype(np.float64)
    x64, a64 = ref.csd_terms64(spec)
    err4, allow4 = np.abs(got - ref.mean64(x64, SIZE_MAX)), BOUND * ref.mean64(a64, SIZE_MAX)
    worst4 = float((err4 / allow4).max())
    print(f"n = {n}: psd {worst:.3f}, csd {worst4:.3f} of the bound")
    assert (err <= allow).all() and (err4 <= allow4).all()


def test_random_rows_stay_far_below_the_bound():
    rng = np.random.default_rng(5)
    for n in (1, 31, 32, 33, 100, 1000):
        mags = rng.random((n, 64, 2), np.float32)
        got = ref.welch_mean(ref.psd_terms(mags), SIZE_MAX).astype(np.float64)
        m64 = ref.mean64(mags.astype(np.float64) ** 2, SIZE_MAX)
        assert float((np.abs(got - m64) / (BOUND * m64)).max()) < 0.15, n


def test_group_one_is_the_identity():
    x = wide_signed((9, 33, 4), 9) + np.float32(0.0)
    assert np.array_equal(ref.welch_mean(x, 1).view(np.uint32), x.view(np.uint32))
    mags = np.abs(wide_signed((9, 33, 2), 10))
    assert np.array_equal(ref.welch_mean(ref.psd_terms(mags), 1).view(np.uint32), (mags * mags).view(np.uint32))


def test_equal_channels_give_three_equal_terms_and_plus_zero():
    spec = wide_signed((40, 17, 2, 2), 11)
    spec[:, :, 1] = spec[:, :, 0]
    out = ref.welch_mean(ref.csd_terms(spec), 33).view(np.uint32)
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2]) and (out[..., 3] == 0).all()


F = 80
GROUPS = [1, 31, 32, 33, 70, F, F + 10, SIZE_MAX]


@pytest.mark.parametrize("group", GROUPS)
def test_blocks_and_columns(group):
    geo = ref.Geometry(F, group)
    cols = ref.columns_of(F, group)
    assert geo.columns() == len(cols) == -(-F // min(group, F))
    blocks = [(j, b) for j, (c0, c1) in enumerate(cols) for b in ref.blocks_of(c0, c1)]
    assert geo.blocks() == len(blocks)
    for b, (j, (f0, f1)) in enumerate(blocks):
        assert b // geo.bpc == j                                                  # block to column
        assert (geo.block_first(b), geo.block_end(b)) == (f0, f1)
        assert 1 <= f1 - f0 <= BLOCK
        assert (f0 - cols[j][0]) % BLOCK == 0                                     # counted from the column's first frame
    for j, (c0, c1) in enumerate(cols):
        assert geo.column_end(j) == c1
        last = geo.column_block_end(j) - 1
        assert geo.block_end(last) == c1 and last // geo.bpc == j
        assert geo.block_end(last) - geo.block_first(last) == (c1 - c0 - 1) % BLOCK + 1      # the last short block
    if group >= F:
        assert geo.columns() == 1 and geo.g == F


@pytest.mark.parametrize("own_rows", [True, False])
@pytest.mark.parametrize("cap", [1, 2, 3, 5, 33, 34, 66, 100, 12288])
@pytest.mark.parametrize("group", GROUPS)
def test_ranges_of_the_host_dispatch(group, cap, own_rows):
    """every block once and in order; ranges end on block boundaries; whole columns unless one column is carried alone; the rows and the
    partials of a range fit the workspace wherever a block of rows and one partial row do"""
    geo = ref.Geometry(F, group)
    ranges, (slots, per, carried) = ref.plan(F, group, cap, own_rows)
    nxt = 0
    for b, m, pieces in ranges:
        assert b == nxt and 1 <= m <= per
        nxt = b + m
        f_lo, f_hi = geo.block_first(b), geo.block_end(b + m - 1)
        assert pieces[0][0] == f_lo and sum(k for _, k, _ in pieces) == f_hi - f_lo
        assert [r for _, _, r in pieces] == [False] + [True] * (len(pieces) - 1)
        if own_rows:
            assert all(k <= slots for _, k, _ in pieces)
        if len(pieces) > 1:
            assert m == 1                                                         # only a single block is ever taken in pieces
        j0, j1 = b // geo.bpc, (b + m - 1) // geo.bpc
        if carried:
            assert j0 == j1                                                       # a carried column is alone in its ranges
        else:
            assert b == j0 * geo.bpc and b + m == geo.column_block_end(j1)        # whole columns
    assert nxt == geo.blocks()
    fpb = min(geo.g, BLOCK)
    if not own_rows or cap >= fpb + 1:
        assert slots + per <= max(cap, 1)
    else:
        assert slots + per <= max(cap, 2)
