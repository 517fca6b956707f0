"""The definition of sgx_maxima_batch / sgx_maxima_mags (include/sgx.h) in numpy: per row m[0 .. M-1] of one side

    candidate   an interior j (1 <= j <= M - 2) with m[j] > m[j-1], m[j] >= m[j+1] and m[j] >= floor
    order       descending m[j], ties by ascending j; the first K
    record      ((float)(j + 1), m[j-1], m[j], m[j+1]); slots beyond the candidates hold (0, 0, 0, 0)

as two masks and a lexsort on (-m, j).  `maxima_loop` is the same in a plain Python loop: tests/test_maxima_reference.py holds the two
together bit for bit.  Rows are float32 and finite, >= 0 (the library's own rows); nothing here rounds: every output value is a copy."""
import numpy as np

K_MAX = 64


def maxima_row(m, k, floor=0.0):
    """one row, one side: float32 [M] -> float32 [k][4]"""
    m = np.ascontiguousarray(m, dtype=np.float32)
    out = np.zeros((k, 4), np.float32)
    M = m.shape[0]
    if M < 3:
        return out
    c = m[1:-1]
    mask = (c > m[:-2]) & (c >= m[2:]) & (c >= np.float32(floor))
    j = np.nonzero(mask)[0] + 1
    order = np.lexsort((j, -m[j].astype(np.float64)))[:k]          # the last key is the primary one; -m is exact in float64
    j = j[order]
    n = j.shape[0]
    out[:n, 0] = (j + 1).astype(np.float32)
    out[:n, 1] = m[j - 1]
    out[:n, 2] = m[j]
    out[:n, 3] = m[j + 1]
    return out


def maxima(rows, k, floor=0.0):
    """rows [..., M, 2] of (l, r) magnitudes, as sgx_stft_batch writes them -> [..., 2, k, 4]"""
    rows = np.asarray(rows, dtype=np.float32)
    lead, M = rows.shape[:-2], rows.shape[-2]
    flat = rows.reshape(-1, M, 2)
    out = np.zeros((flat.shape[0], 2, k, 4), np.float32)
    for i in range(flat.shape[0]):
        for s in range(2):
            out[i, s] = maxima_row(flat[i, :, s], k, floor)
    return out.reshape(*lead, 2, k, 4)


def maxima_loop(m, k, floor=0.0):
    """maxima_row without numpy's masks and sort: a Python loop over the bins, then k times the best candidate not yet taken"""
    m = [np.float32(x) for x in m]
    floor = np.float32(floor)
    cands = [j for j in range(1, len(m) - 1) if m[j] > m[j - 1] and m[j] >= m[j + 1] and m[j] >= floor]
    out = np.zeros((k, 4), np.float32)
    for r in range(k):
        best = None
        for j in cands:
            if best is None or m[j] > m[best]:                   # strictly greater: of equal values the lowest j stays
                best = j
        if best is None:
            break
        cands.remove(best)
        out[r] = (np.float32(best + 1), m[best - 1], m[best], m[best + 1])
    return out


def crafted_rows(M, rng=None):
    """{name: float32 [M]} -- the rows on which an implementation of the definition goes wrong: exact ties, plateaus, monotone and
    constant rows, extremes at the ends of the row and beside them.  Some are degenerate where M is small; all are valid rows."""
    rng = rng or np.random.default_rng(M)
    j = np.arange(M)
    rows = {
        "noise": rng.random(M),
        "ties": (j % 2) * 0.5,                                   # every odd j the same value: the order is by j alone
        "ties_two_levels": (j % 2) * (1.0 + (j % 4 == 1)),       # 2, 1, 2, 1 ... on the odd j
        "plateaus": np.repeat(rng.random(M // 3 + 1), 3)[:M],    # runs of three equal values: the leftmost bin of a raised run only
        "rising": (j + 1) / M,
        "falling": (M - j) / M,
        "zero": np.zeros(M),
        "constant": np.full(M, 0.25),
        "ends_larger": np.where((j == 0) | (j == M - 1), 9.0, rng.random(M)),   # never candidates, but neighbour values
        "ends_as_neighbours": np.where((j == 0) | (j == M - 1), 9.0, np.where((j == 1) | (j == M - 2), 10.0, rng.random(M))),
        "strongest_at_1": np.where(j == 1, 5.0, rng.random(M) * 0.5),
        "strongest_at_last_interior": np.where(j == M - 2, 5.0, rng.random(M) * 0.5),
        "few": np.where((j == M // 2) | (j == M // 3), 1.0 + j / M, 0.0),       # fewer candidates than most K
        "quantised": np.floor(rng.random(M) * 4.0) / 4.0,        # four levels: ties and plateaus everywhere
    }
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in rows.items()}
