"""The flux of a bank (include/sgx.h: sgx_flux_batch, sgx_flux_mags) on the host, bit for bit: written from the header's text
alone, in numpy, with no GPU and no torch.

Per frame t, pair, side and stored bin j
    x_t[j] = m (power 1) or rn(m * m) (power 2)          tests/fbank_reference.py: elements
    d[j]   = rn(x_t[j] - x_{t - lag}[j])                  one float32 subtract
    rise   = d < 0 ? +0 : d,    fall = d > 0 ? +0 : rn(+0 - d)
and per filter the four sums (rise_l, rise_r, fall_l, fall_r) in the order of the filterbank sums (64 fused multiply-add chains from +0,
then the tree by halving: tests/fbank_reference.py: _sums).  A frame t < lag has no predecessor: its records are +0.

flux_plain is the same in plain Python loops, one scalar at a time; the two mutants are what a caller would compute from outputs the
library already has, and what a kernel that squares after the subtract would: the tests show that their inputs tell them apart."""
import numpy as np

import fbank_reference as fr

MAX_LAG = 64
WORKSPACE_BYTES = 192 << 20


def rise_fall(x, lag):
    """x [frames][pairs][M][2] float32 elements -> (rise, fall), same shape; frames t < lag are +0"""
    x = np.asarray(x, np.float32)
    rise, fall = np.zeros_like(x), np.zeros_like(x)
    if x.shape[0] > lag:
        with np.errstate(invalid="ignore", over="ignore"):
            d = (x[lag:] - x[:-lag]).astype(np.float32)
            rise[lag:] = np.where(d < 0, np.float32(0.0), d)
            fall[lag:] = np.where(d > 0, np.float32(0.0), (np.float32(0.0) - d).astype(np.float32))
    return rise, fall


def flux(rows, bank, power, lag, watch=None):
    """rows [frames][pairs][M][2] float32 (what sgx_stft_batch stores) -> [frames][pairs][n_filters][4] float32: sgx_flux_mags to
    the bit"""
    assert 1 <= lag <= MAX_LAG
    rows = np.asarray(rows, np.float32)
    assert rows.ndim == 4 and rows.shape[-1] == 2
    rise, fall = rise_fall(fr.elements(rows, power), lag)
    e = np.concatenate([rise, fall], -1)                   # [frames][pairs][M][4]: (rise_l, rise_r, fall_l, fall_r)
    if watch is not None:
        watch(e)
    out = np.zeros(rows.shape[:2] + (len(bank[0]), 4), np.float32)      # no predecessor: +0 whatever the rows hold, NaN included
    if rows.shape[0] > lag:
        with np.errstate(invalid="ignore", over="ignore"):
            out[lag:] = fr._sums(e[lag:], bank, watch)
    return out


def flux_of(cur, prev, bank, power):
    """the records of the frames `cur` [n][pairs][M][2] whose predecessors are `prev`, same shape -> [n][pairs][n_filters][4]: flux() on
    chosen frames of a long call"""
    cur, prev = np.asarray(cur, np.float32), np.asarray(prev, np.float32)
    assert cur.shape == prev.shape and cur.ndim == 4
    out = np.zeros(cur.shape[:2] + (len(bank[0]), 4), np.float32)
    for i in range(cur.shape[0]):                          # (frame by frame: any lag, any number of frames)
        out[i] = flux(np.stack([prev[i], cur[i]]), bank, power, 1)[1]
    return out


def flux_float64(rows, bank, power, lag):
    """the same quantities in float64, no rounding order to speak of: the truth the arithmetic bound is held against"""
    first, count, weights = bank
    x = np.asarray(rows, np.float64) ** power
    d = np.zeros_like(x)
    d[lag:] = x[lag:] - x[:-lag]
    e = np.concatenate([np.maximum(d, 0.0), np.maximum(-d, 0.0)], -1)
    off = fr._offsets(count)
    w = np.asarray(weights, np.float64)
    out = np.zeros(e.shape[:2] + (len(first), 4))
    for f in range(len(first)):
        j, c = int(first[f]), int(count[f])
        out[:, :, f, :] = np.einsum("i,tpiq->tpq", w[off[f]:off[f + 1]], e[:, :, j:j + c, :])
    return out


def arithmetic_bound(rows, bank, power, lag):
    """what |float32 flux - float64 flux of the same float32 rows| may be, per (frame, pair, filter, side):
    (ceil(count / 64) + 9) * 2^-24 * sum_i |w_i| (x_t[j] + x_{t - lag}[j]) -- one rounding for the square, one for the subtract, the chain,
    six tree levels and one for second order.  [frames][pairs][n_filters][2]; frames t < lag are 0."""
    first, count, weights = bank
    x = np.abs(np.asarray(rows, np.float64)) ** power
    s = np.zeros_like(x)
    s[lag:] = x[lag:] + x[:-lag]
    off = fr._offsets(count)
    w = np.abs(np.asarray(weights, np.float64))
    out = np.zeros(s.shape[:2] + (len(first), 2))
    for f in range(len(first)):
        j, c = int(first[f]), int(count[f])
        out[:, :, f, :] = (-(-c // 64) + 9) * 2.0 ** -24 * np.einsum("i,tpiq->tpq", w[off[f]:off[f + 1]], s[:, :, j:j + c, :])
    return out


# ---- the same in plain loops ------------------------------------------------------------------------------------------------------------
def flux_plain(rows, bank, power, lag):
    """flux() one scalar at a time: Python loops over frames, pairs, filters, components, lanes and tree levels"""
    f32 = np.float32
    rows = np.asarray(rows, f32)
    first, count, weights = bank
    weights = np.asarray(weights, f32)
    off = fr._offsets(count)
    T, P, M, _ = rows.shape
    out = np.zeros((T, P, len(first), 4), f32)
    zero = f32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(lag, T):
            for p in range(P):
                e = np.zeros((M, 4), f32)
                for j in range(M):
                    for s in range(2):
                        a, b = rows[t, p, j, s], rows[t - lag, p, j, s]
                        if power == 2:
                            a, b = f32(a * a), f32(b * b)
                        d = f32(a - b)
                        e[j, s] = zero if d < 0 else d
                        e[j, 2 + s] = zero if d > 0 else f32(zero - d)
                for f in range(len(first)):
                    c, j0 = int(count[f]), int(first[f])
                    if c == 0:
                        continue
                    for q in range(4):
                        a = [zero] * fr.LANES
                        for i in range(c):
                            a[i % fr.LANES] = fr.fma32(weights[off[f] + i], e[j0 + i, q], a[i % fr.LANES]).reshape(())[()]
                        for s in fr.LEVELS:
                            a = [f32(a[l] + a[l + s]) for l in range(s)]
                        out[t, p, f, q] = a[0]
    return out


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
def mutant_band_difference(rows, bank, power, lag):
    """the difference of two sgx_fbank_batch columns, rectified per band: rising and falling partials of a band cancel"""
    rows = np.asarray(rows, np.float32)
    sums = fr.bank_sums(rows, bank, power)                 # [frames][pairs][n_filters][2]
    rise, fall = rise_fall(sums, lag)
    return np.concatenate([rise, fall], -1)


def mutant_square_after(rows, bank, power, lag):
    """the subtract before the square: rn(rn(m_t - m_{t - lag})^2), signed like the difference"""
    rows = np.asarray(rows, np.float32)
    d = np.zeros_like(rows)
    d[lag:] = (rows[lag:] - rows[:-lag]).astype(np.float32)
    if power == 2:
        d = (np.sign(d) * (d * d).astype(np.float32)).astype(np.float32)
    rise = np.where(d < 0, np.float32(0.0), d)
    fall = np.where(d > 0, np.float32(0.0), (np.float32(0.0) - d).astype(np.float32))
    out = fr._sums(np.concatenate([rise, fall], -1), bank, None)
    out[:lag] = 0.0
    return out


# ---- the host's range arithmetic restated (csrc/flux_host.hpp) ---------------------------------------------------------------------------
def max_lag(row_bytes):
    cap = WORKSPACE_BYTES // row_bytes
    return 0 if cap < 2 else min(MAX_LAG, cap - 1)


def flux_stage_staged(M, lds_optin=fr.STAGE_LDS_CAP):
    """launch_fbank_flux_stage: the two float2 columns of a frame in LDS (the cross stage's threshold), or both rows read where they lie"""
    return fr.cross_stage_staged(M, lds_optin)


# ---- rows and banks of the tests ----------------------------------------------------------------------------------------------------------
def ones_bank(M):
    return np.zeros(1, np.uint32), np.array([M], np.uint32), np.ones(M, np.float32)


def empty_bank(M, n=5):
    first = np.array([0, M, M // 2, 0, M][:n], np.uint32)
    return first, np.zeros(n, np.uint32), np.zeros(0, np.float32)
