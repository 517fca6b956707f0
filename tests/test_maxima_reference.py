"""tests/maxima_reference.py (the numpy restatement of include/sgx.h's spectral maxima) against a plain Python loop, bit for bit, and on
rows whose answer is known by hand.  No GPU."""
import numpy as np
import pytest

import maxima_reference as ref

KS = (1, 2, 5, 64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("M", [1, 2, 3, 5, 64, 257, 2047])
def test_masks_and_lexsort_equal_the_loop_on_random_rows(M):
    rng = np.random.default_rng(1000 + M)
    for trial in range(4):
        m = rng.random(M).astype(np.float32)
        if trial == 3:
            m = (np.floor(m * 8.0) / 8.0).astype(np.float32)      # ties and plateaus
        for k in KS:
            for floor in (0.0, 0.5, float(np.sort(m)[M // 2])):
                assert same_bits(ref.maxima_row(m, k, floor), ref.maxima_loop(m, k, floor)), (M, trial, k, floor)


@pytest.mark.parametrize("M", [3, 5, 255, 256, 257])
def test_masks_and_lexsort_equal_the_loop_on_crafted_rows(M):
    for name, m in ref.crafted_rows(M).items():
        for k in KS:
            for floor in (0.0, 0.25):
                assert same_bits(ref.maxima_row(m, k, floor), ref.maxima_loop(m, k, floor)), (M, name, k, floor)


def test_exact_ties_are_ordered_by_bin():
    m = np.array([0, 2, 0, 2, 0, 3, 0, 2, 0], np.float32)
    got = ref.maxima_row(m, 5)
    assert got[:, 0].tolist() == [6.0, 2.0, 4.0, 8.0, 0.0]        # bins k = j + 1: the 3 first, then the 2s by ascending bin
    assert got[0].tolist() == [6.0, 0.0, 3.0, 0.0] and got[4].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert ref.maxima_row(m, 2)[:, 0].tolist() == [6.0, 2.0]


def test_a_plateau_yields_its_leftmost_bin_only():
    # j = 1 of (1, 1, 1) and j = 5 of (2, 2) rise from the left and are >= the right; j = 8 rises from m[7] = 0 and m[9] equals it: a
    # candidate too, although j = 9 itself can never be one
    m = np.array([0, 1, 1, 1, 0, 2, 2, 0, 0.5, 0.5], np.float32)
    got = ref.maxima_row(m, 4)
    assert got.tolist() == [[6.0, 0.0, 2.0, 2.0], [2.0, 0.0, 1.0, 1.0], [9.0, 0.0, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0]]
    assert ref.maxima_row(np.array([0, 0.5, 0.5], np.float32), 1)[0].tolist() == [2.0, 0.0, 0.5, 0.5]
    assert not ref.maxima_row(np.array([0.5, 0.5, 0], np.float32), 1).any()       # the plateau begins at bin 1: its left edge is not stored


def test_monotone_constant_and_zero_rows_have_no_maximum():
    for M in (3, 5, 64):
        rows = ref.crafted_rows(M)
        for name in ("rising", "falling", "zero", "constant"):
            assert not ref.maxima_row(rows[name], 5).any(), (M, name)


def test_the_ends_are_never_candidates_but_are_neighbours():
    # the largest values sit at j = 0 and j = M - 1: ignored as candidates, and they keep j = 1 and j = 3 from being any
    assert not ref.maxima_row(np.array([20, 10, 0, 5, 30], np.float32), 3).any()
    # as neighbour values they appear in the records of j = 1 and j = M - 2
    got = ref.maxima_row(np.array([9, 10, 0, 0, 0, 5, 4], np.float32), 3)
    assert got.tolist() == [[2.0, 9.0, 10.0, 0.0], [6.0, 0.0, 5.0, 4.0], [0.0, 0.0, 0.0, 0.0]]


def test_floor_equal_to_a_candidate_and_one_ulp_above():
    m = np.array([0, 0.75, 0, 0.5, 0, 0.25, 0], np.float32)
    half = np.float32(0.5)
    assert ref.maxima_row(m, 3, float(half))[:, 0].tolist() == [2.0, 4.0, 0.0]                 # m >= floor keeps the equal one
    above = np.nextafter(half, np.float32(1.0))
    assert ref.maxima_row(m, 3, float(above))[:, 0].tolist() == [2.0, 0.0, 0.0]
    assert ref.maxima_row(m, 3, 0.0)[:, 0].tolist() == [2.0, 4.0, 6.0]


def test_fewer_candidates_than_k_and_short_rows():
    m = np.array([0, 1, 0, 0, 0], np.float32)
    got = ref.maxima_row(m, 64)
    assert got.shape == (64, 4) and got[0].tolist() == [2.0, 0.0, 1.0, 0.0] and not got[1:].any()
    for M in (1, 2):
        assert not ref.maxima_row(np.ones(M, np.float32), 5).any()
    assert ref.maxima_row(np.array([0, 1, 0], np.float32), 2)[:, 0].tolist() == [2.0, 0.0]      # M = 3: one interior bin
    assert ref.maxima_row(np.array([0, 1, 0, 2, 0], np.float32), 2)[:, 0].tolist() == [4.0, 2.0]


def test_rows_of_both_sides():
    rng = np.random.default_rng(5)
    rows = rng.random((3, 2, 17, 2)).astype(np.float32)
    got = ref.maxima(rows, 4, 0.1)
    assert got.shape == (3, 2, 2, 4, 4)
    for f in range(3):
        for p in range(2):
            for s in range(2):
                assert same_bits(got[f, p, s], ref.maxima_loop(rows[f, p, :, s], 4, 0.1))
