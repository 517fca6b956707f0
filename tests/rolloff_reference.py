"""The definition of sgx_rolloff_batch / sgx_rolloff_mags (include/sgx.h) in numpy: per row m[0 .. M-1] of one side

    summand     x[j] = m[j] (power 1) or rn(m[j] * m[j]) (power 2)
    segments    of S = 32 consecutive elements from element 0; s[b][i] = rn(s[b][i-1] + x[32 b + i]) from +0
    offsets     o[0] = +0, o[b+1] = rn(o[b] + s[b][last])
    cumulative  c[32 b + i] = rn(o[b] + s[b][i]); T = c[M-1]
    record      per share p: thr = rn(p * T), j* the smallest j with c[j] >= thr: ((float)(j* + 1), c[j*-1], c[j*], T), +0 for c[-1];
                (0, 0, 0, T) where !(T > 0)

as a pad to whole segments with +0 (which changes no sum), np.cumsum along the segments, np.cumsum of the segment totals shifted by one,
and one add.  `cumulative_loop` and `rolloff_loop` are the same in a plain Python loop of np.float32 scalars:
tests/test_rolloff_reference.py holds the two together bit for bit.  Rows are float32 and >= +0 (the library's own rows), or hold NaN."""
import numpy as np

S = 32
P_MAX = 8


def _summands(rows, power):
    rows = np.asarray(rows, dtype=np.float32)
    if power == 1:
        return rows
    if power == 2:
        with np.errstate(invalid="ignore", over="ignore"):
            return rows * rows                                   # float32 * float32: one rounding
    raise ValueError("power must be 1 or 2")


def cumulative(rows, power):
    """rows [..., M, 2] of (l, r) magnitudes, as sgx_stft_batch writes them -> c [..., M, 2] float32"""
    x = np.moveaxis(_summands(rows, power), -1, -2)              # [..., 2, M]
    lead, M = x.shape[:-1], x.shape[-1]
    nb = -(-M // S)
    padded = np.zeros(lead + (nb * S,), np.float32)
    padded[..., :M] = x
    with np.errstate(invalid="ignore", over="ignore"):
        seg = np.cumsum(padded.reshape(lead + (nb, S)), axis=-1, dtype=np.float32)
        off = np.zeros(lead + (nb,), np.float32)
        off[..., 1:] = np.cumsum(seg[..., -1], axis=-1, dtype=np.float32)[..., :-1]
        c = (off[..., None] + seg).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(c.reshape(lead + (nb * S,))[..., :M], -2, -1))


def rolloff(rows, power, p):
    """rows [..., M, 2] -> records [..., 2, n_p, 4] float32"""
    p = np.atleast_1d(np.asarray(p, dtype=np.float32))
    assert 1 <= p.shape[0] <= P_MAX and ((p > 0) & (p <= 1)).all()
    c = np.moveaxis(cumulative(rows, power), -1, -2)             # [..., 2, M]
    total = c[..., -1]
    out = np.zeros(c.shape[:-1] + (p.shape[0], 4), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        live = total > 0
        for i, share in enumerate(p):
            thr = (share * total).astype(np.float32)             # one float32 product
            j = np.argmax(c >= thr[..., None], axis=-1)          # the first j that reaches it (0 where none does: not live)
            at = np.take_along_axis(c, j[..., None], -1)[..., 0]
            below = np.where(j > 0, np.take_along_axis(c, np.maximum(j - 1, 0)[..., None], -1)[..., 0], np.float32(0))
            out[..., i, 0] = np.where(live, (j + 1).astype(np.float32), np.float32(0))
            out[..., i, 1] = np.where(live, below, np.float32(0))
            out[..., i, 2] = np.where(live, at, np.float32(0))
            out[..., i, 3] = total
    return out


def cumulative_loop(m, power):
    """cumulative() for one side of one row, float32 [M] -> [M], as the definition reads: np.float32 scalars, one operation at a time"""
    zero = np.float32(0)
    m = [np.float32(v) for v in m]
    c, o = [], zero
    with np.errstate(invalid="ignore", over="ignore"):
        x = m if power == 1 else [v * v for v in m]
        for b in range(0, len(x), S):
            s = zero
            for v in x[b:b + S]:
                s = np.float32(s + v)
                c.append(np.float32(o + s))
            o = np.float32(o + s)
    return np.array(c, np.float32)


def rolloff_loop(m, power, p):
    """rolloff() for one side of one row: float32 [M] -> [n_p][4]"""
    c = cumulative_loop(m, power)
    total = c[-1]
    out = np.zeros((len(p), 4), np.float32)
    out[:, 3] = total
    if not total > 0:
        return out
    for i, share in enumerate(p):
        thr = np.float32(np.float32(share) * total)
        j = next(j for j in range(len(c)) if c[j] >= thr)
        out[i, :3] = (np.float32(j + 1), c[j - 1] if j else np.float32(0), c[j])
    return out


def crafted_rows(M, rng=None):
    """{name: float32 [M]} -- rows known by hand, rows that put all their weight on a segment's or a tile's first and last element, and
    random rows.  Some coincide where M is small; all are valid rows (>= +0, or a NaN)."""
    rng = rng or np.random.default_rng(M)
    j = np.arange(M)
    h = rng.random(M) + 0.5
    nan_row = rng.random(M)
    nan_row[M // 2] = np.nan
    rows = {
        "ones": np.ones(M),
        "only_first": np.where(j == 0, 3.0, 0.0),
        "only_last": np.where(j == M - 1, 3.0, 0.0),
        "only_31": np.where(j == min(31, M - 1), 3.0, 0.0),
        "only_32": np.where(j == min(32, M - 1), 3.0, 0.0),
        "zero": np.zeros(M),
        "nan_in_the_middle": nan_row,
        "huge_first": np.where(j == 0, 1e30, 1.0),
        "segment_ends": np.where(j % S == S - 1, h, 0.0),
        "segment_starts": np.where(j % S == 0, h, 0.0),
        "tile_ends": np.where((j % 2048 == 0) | (j % 2048 == 2047), h, 0.0),
        "noise": rng.random(M),
        "noise_wide": rng.random(M) * np.exp(6.0 * rng.random(M)),
        "falling": (M - j) / M,
    }
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in rows.items()}
