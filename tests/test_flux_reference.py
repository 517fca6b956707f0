"""tests/flux_reference.py, without a GPU: the host restatement of the flux of a bank (include/sgx.h: sgx_flux_batch) is held to a
plain Python loop, to rows known by hand, and to the properties the GPU tests rely on -- equal rows give +0 and never -0, a NaN bin
shows in the filters that cover it and in no other, the first `lag` frames are zero, pairs do not mix, and its inputs tell it apart from
the two things a caller or a faulty kernel would compute instead."""
import numpy as np
import pytest

import fbank_reference as fr
import flux_reference as ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def small_rows(frames, pairs, M, seed):
    return fr.synthetic_mags(frames * pairs, M, seed).reshape(frames, pairs, M, 2)


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("lag", [1, 3])
def test_equals_the_plain_loop(power, lag):
    M = 70                                                  # filters of more than 64 bins: the chains go on
    rows = small_rows(lag + 3, 2, M, seed=11 * lag + power)
    rows[lag + 1] = rows[1]                                 # a frame equal to its predecessor
    rows[-1, 1, 5, 0] = np.nan
    bank = fr.edge_bank(M)
    got, want = ref.flux(rows, bank, power, lag), ref.flux_plain(rows, bank, power, lag)
    assert got.shape == (lag + 3, 2, fr.N_EDGE_FILTERS, 4)
    nan = np.isnan(want)
    assert nan.any() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("power", [1, 2])
def test_rows_known_by_hand(power):
    """small integers and an all-ones filter: every operation is exact"""
    M = 9
    rows = np.zeros((3, 1, M, 2), np.float32)
    rows[0, 0, :, 0] = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    rows[1, 0, :, 0] = [3, 2, 1, 4, 9, 0, 7, 10, 8]
    rows[2, 0, :, 0] = [0, 0, 0, 0, 0, 0, 0, 0, 0]
    rows[..., 1] = rows[::-1, :, :, 0]                      # the right side runs backwards in time
    out = ref.flux(rows, ref.ones_bank(M), power, 1)
    x = rows.astype(np.int64) ** power
    for t in (1, 2):
        d = x[t, 0] - x[t - 1, 0]                           # [M][2]
        rise, fall = np.maximum(d, 0).sum(0), np.maximum(-d, 0).sum(0)
        assert out[t, 0, 0].tolist() == [rise[0], rise[1], fall[0], fall[1]]
        assert (out[t, 0, 0, :2] - out[t, 0, 0, 2:]).tolist() == (x[t, 0].sum(0) - x[t - 1, 0].sum(0)).tolist()    # rise - fall telescopes
    if power == 1:
        assert out[1, 0, 0].tolist() == [2 + 4 + 2, 3 + 2 + 1 + 4 + 9 + 0 + 7 + 10 + 8, 2 + 6 + 1, 0]    # (right: frame 1 against zeros)
    # lag 2 skips the middle frame
    out2 = ref.flux(rows, ref.ones_bank(M), power, 2)
    assert out2[2, 0, 0].tolist() == [0, float(x[0, 0, :, 0].sum()), float(x[0, 0, :, 0].sum()), 0]
    assert not out2[:2].any()


@pytest.mark.parametrize("power", [1, 2])
def test_equal_rows_give_plus_zero(power):
    M = 65
    rows = small_rows(4, 2, M, seed=3)
    rows[1:] = rows[0]
    rows[:, 0, 7, :] = 0.0
    rows[:, 1, 9, :] = -0.0                                 # (no magnitude is -0; equal words still give +0)
    out = ref.flux(rows, fr.edge_bank(M), power, 1)
    assert not bits(out).any(), "equal rows do not give +0 everywhere"


def test_a_nan_bin_shows_in_its_filters_alone():
    M, lag = 130, 2
    rows = small_rows(5, 2, M, seed=5)
    clean = ref.flux(rows, fr.edge_bank(M), 2, lag)
    rows[3, 1, 64, 0] = np.nan                              # frame 3 as itself, frame 5 would be its successor: only (3, pair 1, left)
    first, count, _ = bank = fr.edge_bank(M)
    out = ref.flux(rows, bank, 2, lag)
    covers = (first <= 64) & (64 < first.astype(np.int64) + count)
    assert covers.sum() >= 3 and (~covers).sum() >= 200
    want_nan = np.zeros(out.shape, bool)
    want_nan[3, 1, covers, 0] = want_nan[3, 1, covers, 2] = True      # rise_l and fall_l, both
    assert np.array_equal(np.isnan(out), want_nan)
    assert np.array_equal(bits(out)[~want_nan], bits(clean)[~want_nan])
    # as a predecessor it shows lag frames later
    rows5 = np.concatenate([rows, rows[:2]])
    out5 = ref.flux(rows5, bank, 2, lag)
    assert np.isnan(out5[5, 1, covers, 0]).all() and np.isnan(out5[5, 1, covers, 2]).all() and not np.isnan(out5[5, 0]).any()


@pytest.mark.parametrize("lag", [1, 2, 5, 64])
def test_the_first_lag_frames_are_zero(lag):
    M = 7
    for frames in (1, lag, lag + 1, lag + 6):
        rows = small_rows(frames, 2, M, seed=lag)
        rows[0, 0, 0, 0] = np.nan                           # nothing of a frame without a predecessor is read
        out = ref.flux(rows, fr.edge_bank(M), 1, lag)
        assert out.shape[0] == frames and not bits(out[:lag]).any()
        if frames > lag + 1:
            assert out[lag + 1:].any() and not np.isnan(out[lag + 1:]).any()


def test_pairs_do_not_mix():
    M, lag = 33, 1
    rows = small_rows(4, 3, M, seed=8)
    bank = fr.edge_bank(M)
    out = ref.flux(rows, bank, 2, lag)
    for p in range(3):
        alone = ref.flux(rows[:, p:p + 1], bank, 2, lag)
        assert np.array_equal(bits(out[:, p:p + 1]), bits(alone))
    swapped = ref.flux(rows[:, ::-1], bank, 2, lag)
    assert np.array_equal(bits(swapped), bits(out[:, ::-1])) and not np.array_equal(bits(out[:, 0]), bits(out[:, 1]))
    # nor do the sides
    flipped = ref.flux(rows[..., ::-1], bank, 2, lag)
    assert np.array_equal(bits(flipped), bits(out[..., [1, 0, 3, 2]]))


@pytest.mark.parametrize("power", [1, 2])
def test_differs_from_the_mutants(power):
    M, lag = 255, 1
    rows = small_rows(4, 1, M, seed=21)
    bank = fr.edge_bank(M)
    out = ref.flux(rows, bank, power, lag)
    wide = bank[1] >= 2                                     # a filter of one bin cannot tell: its band sum is its bin
    # differencing the band sums: rise and fall of a band are never both positive there, here they are on every wide filter
    band = ref.mutant_band_difference(rows, bank, power, lag)
    assert not ((band[..., :2] > 0) & (band[..., 2:] > 0)).any()
    both = (out[lag:, :, :, :2] != 0) & (out[lag:, :, :, 2:] != 0)
    assert both[:, :, bank[1] >= 63].all()
    assert (bits(out[lag:][:, :, wide]) != bits(band[lag:][:, :, wide])).mean() > 0.9
    # differencing before squaring
    after = ref.mutant_square_after(rows, bank, power, lag)
    if power == 1:
        assert np.array_equal(bits(after), bits(out))       # (nothing to square: the mutant is the definition)
    else:
        nz = out[lag:] != 0
        assert (bits(out[lag:])[nz] != bits(after[lag:])[nz]).mean() > 0.9


def test_float64_truth_and_the_arithmetic_bound():
    """the reference alone stays well inside the bound the GPU test holds the device to"""
    for M in (3, 255):
        for lag in (1, 3):
            for power in (1, 2):
                rows = small_rows(lag + 4, 2, M, seed=M + lag)
                bank = fr.edge_bank(M)
                err = np.abs(ref.flux(rows, bank, power, lag).astype(np.float64) - ref.flux_float64(rows, bank, power, lag))
                bound = ref.arithmetic_bound(rows, bank, power, lag)
                bound4 = np.concatenate([bound, bound], -1)
                assert (err <= bound4).all()
                worst = float((err[bound4 > 0] / bound4[bound4 > 0]).max())
                print(f"M {M}, lag {lag}, power {power}: worst error / bound = {worst:.3f}")
                assert worst <= 0.5


def test_max_lag_restated():
    assert ref.max_lag(1 * 2047 * 8) == 64                  # W 2048, two channels
    assert ref.max_lag(1 * (2 ** 20 - 1) * 8) == 23         # W 2^20, two channels
    assert ref.max_lag(2 * (2 ** 20 - 1) * 8) == 11         # W 2^20, four channels
    assert ref.max_lag((96 << 20) + 8) == 0
    assert ref.flux_stage_staged(10240) and not ref.flux_stage_staged(10241)
