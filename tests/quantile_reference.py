"""The definition of sgx_quantile_batch / sgx_quantile_mags (include/sgx.h) restated in numpy: the key that orders float32 words, a sort
along the frame axis, the rank rule, the key's inverse.  Also the host's range arithmetic of the batch call (spectrogram_rs_amd/csrc/
sgx_api.hip), so that the GPU tests know where the workspace's seams fall.

tests/test_quantile_reference.py holds this file to a plain Python loop bit for bit and to results known by hand."""
import math

import numpy as np

MAX_Q = 16                              # include/sgx.h: n_q from 1 to 16
WORKSPACE_BYTES = 192 << 20             # include/sgx.h: the bounded workspace
SIZE_MAX = 2 ** 64 - 1


def key(u):
    """uint32 bit patterns -> the keys whose unsigned order is -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN"""
    u = np.asarray(u, dtype=np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def rank(q, n):
    """floor(q * (double)(n - 1) + 0.5): one double product, one add, one floor"""
    return int(math.floor(float(q) * float(n - 1) + 0.5))


def columns(n_frames, group):
    """[(first frame, frames)] of every column; the last one may be short"""
    g = min(group, n_frames)
    return [(f, min(g, n_frames - f)) for f in range(0, n_frames, g)] if n_frames else []


def quantiles_of_sets(rows, group, qsets):
    """quantiles() for several sets of q over the same rows: every column is sorted once"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert all(1 <= len(q) <= MAX_Q for q in qsets) and group >= 1
    words = rows.view(np.uint32)
    cols = columns(rows.shape[0], group)
    outs = [np.empty((len(cols), len(q)) + rows.shape[1:], dtype=np.uint32) for q in qsets]
    for j, (f, n) in enumerate(cols):
        ordered = np.sort(key(words[f:f + n]), axis=0)
        for out, q in zip(outs, qsets):
            for i, qi in enumerate(q):
                out[j, i] = unkey(ordered[rank(qi, n)])
    return [out.view(np.float32) for out in outs]


def quantiles(rows, group, q):
    """float32 rows [frames][...] -> [columns][n_q][...]: per column and flat element the words of the ranks of q among the column's frames"""
    return quantiles_of_sets(rows, group, [q])[0]


def valid_q(q):
    return 1 <= len(q) <= MAX_Q and all(0.0 <= x <= 1.0 for x in q)      # (a NaN fails both comparisons)


def cap(row_bytes):
    """sgx_quantile_max_group: the frames of rows the workspace holds, at least 1"""
    return max(WORKSPACE_BYTES // row_bytes, 1)


def plan(n, group, row_bytes):
    """The ranges sgx_quantile_batch takes n frames in: [(first frame, frames, first column)], whole columns each, or None where the call is
    refused (a column longer than the cap)"""
    g = min(group, n)
    c = cap(row_bytes)
    if g > c:
        return None
    per = c // g * g
    return [(f, min(per, n - f), f // g) for f in range(0, n, per)]
