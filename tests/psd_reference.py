"""The host reference of sgx_psd_batch / sgx_csd_batch (include/sgx.h), and the block / column / range arithmetic of the host dispatch
mirrored in Python from the header's words.

The definition: a call's F frames fall into columns of `group` frames (the last may be shorter); a column's frames into blocks of 32
consecutive frames counted from the column's first (the last may be shorter); a block's partial is one chain of float32 adds from +0 in
ascending frame order; the column's sum one chain of float64 adds from +0 over its partials; the output (float)(S / (double)n_j).
numpy: a float32 cumsum along the frames of a block, a float64 cumsum over the blocks (np.add.accumulate is one sequential chain;
tests/test_psd_reference.py holds it to a Python loop bit for bit)."""
import numpy as np

BLOCK = 32
SIZE_MAX = 2 ** 64 - 1
BOUND = 35.0 * 2.0 ** -24            # include/sgx.h: times the mean of the absolute products of the term


def columns_of(n, group):
    """[(first, end)] of every column of n frames"""
    assert group >= 1
    g = min(group, n)
    return [(a, min(a + g, n)) for a in range(0, n, g)] if n else []


def blocks_of(first, end):
    """[(first, end)] of every block of a column's frames"""
    return [(a, min(a + BLOCK, end)) for a in range(first, end, BLOCK)]


def chain32(x):
    """one chain of float32 adds from +0 over axis 0"""
    x = np.asarray(x, np.float32)
    zero = np.zeros((1,) + x.shape[1:], np.float32)
    return np.add.accumulate(np.concatenate([zero, x]), axis=0, dtype=np.float32)[-1]


def chain64(p):
    """one chain of float64 adds from +0 over axis 0 of float32 partials"""
    p = np.asarray(p, np.float32).astype(np.float64)
    zero = np.zeros((1,) + p.shape[1:], np.float64)
    return np.add.accumulate(np.concatenate([zero, p]), axis=0, dtype=np.float64)[-1]


def welch_mean(x, group):
    """x [F, ...] float32 summands -> [columns, ...] float32 means, by the definition"""
    x = np.asarray(x, np.float32)
    out = []
    for c0, c1 in columns_of(x.shape[0], group):
        partials = np.stack([chain32(x[b0:b1]) for b0, b1 in blocks_of(c0, c1)])
        out.append((chain64(partials) / np.float64(c1 - c0)).astype(np.float32))
    return np.stack(out) if out else np.zeros((0,) + x.shape[1:], np.float32)


def welch_mean_loop(x, group):
    """the same by a straight Python loop over scalars (slow: small inputs only)"""
    x = np.asarray(x, np.float32)
    flat = x.reshape(x.shape[0], -1)
    cols = columns_of(flat.shape[0], group)
    out = np.zeros((len(cols), flat.shape[1]), np.float32)
    for j, (c0, c1) in enumerate(cols):
        for e in range(flat.shape[1]):
            S = np.float64(0.0)
            for b0, b1 in blocks_of(c0, c1):
                s = np.float32(0.0)
                for f in range(b0, b1):
                    s = np.float32(s + flat[f, e])
                S = np.float64(S + np.float64(s))
            out[j, e] = np.float32(S / np.float64(c1 - c0))
    return out.reshape((len(cols),) + x.shape[1:])


def psd_terms(mags):
    """x = rn(m * m) of magnitude rows, any shape"""
    m = np.asarray(mags, np.float32)
    return (m * m).astype(np.float32)


def csd_terms(spec):
    """x0 .. x3 in numpy float32, every product and the one sum or difference rounded: [..., M, 2, 2] -> [..., M, 4]"""
    s = np.asarray(spec, np.float32)
    a, b, c, d = s[..., 0, 0], s[..., 0, 1], s[..., 1, 0], s[..., 1, 1]
    return np.stack([a * a + b * b, c * c + d * d, a * c + b * d, b * c - a * d], -1).astype(np.float32)


def csd_terms64(spec):
    """the four terms in float64 of the same float32 words, and the sum of the absolute products of each term"""
    s = np.asarray(spec, np.float32).astype(np.float64)
    a, b, c, d = s[..., 0, 0], s[..., 0, 1], s[..., 1, 0], s[..., 1, 1]
    x = np.stack([a * a + b * b, c * c + d * d, a * c + b * d, b * c - a * d], -1)
    m = np.stack([a * a + b * b, c * c + d * d, np.abs(a * c) + np.abs(b * d), np.abs(b * c) + np.abs(a * d)], -1)
    return x, m


def mean64(x64, group):
    """the float64 mean over every column of float64 values [F, ...]"""
    return np.stack([x64[a:b].mean(axis=0) for a, b in columns_of(x64.shape[0], group)])


# ---- the host dispatch's arithmetic (spectrogram_rs_amd/csrc/sgx_psd.hpp: Geometry; sgx_api.hip: psd_reduce) ---------------------------
class Geometry:
    def __init__(self, n, group):
        assert n >= 1 and group >= 1
        self.n, self.g = n, min(group, n)
        self.bpc = -(-self.g // BLOCK)

    def columns(self):
        return (self.n - 1) // self.g + 1

    def blocks(self):
        full, rem = divmod(self.n, self.g)
        return full * self.bpc + -(-rem // BLOCK)

    def column_end(self, j):
        return self.n if self.n - j * self.g < self.g else (j + 1) * self.g

    def block_first(self, b):
        return (b // self.bpc) * self.g + (b % self.bpc) * BLOCK

    def block_end(self, b):
        f, ce = self.block_first(b), self.column_end(b // self.bpc)
        return ce if ce - f < BLOCK else f + BLOCK

    def column_block_end(self, j):
        return self.blocks() if self.blocks() - j * self.bpc < self.bpc else (j + 1) * self.bpc


def plan(n, group, cap, own_rows):
    """The ranges psd_reduce takes a call in: [(first block, blocks, [(first frame, frames, resume)])], with the workspace holding `cap`
    rows (a row and a block's partial row are the same size).  Also answers (row slots, partial slots, carried)."""
    geo = Geometry(n, group)
    fpb = min(geo.g, BLOCK)
    every = geo.blocks()
    per, piece = cap, None
    if own_rows:
        if cap >= fpb + 1:
            per = cap // (fpb + 1)
        else:
            per, piece = 1, max(cap - 1, 1)
    per = min(max(per, 1), every)
    carried = geo.bpc > per
    if not carried:
        per -= per % geo.bpc
    slots = min(piece if piece is not None else per * fpb, n) if own_rows else 0
    ranges, b = [], 0
    while b < every:
        j = b // geo.bpc
        m = min(every - b, per)
        if carried:
            m = min(m, geo.column_block_end(j) - b)
        f_lo, f_hi = geo.block_first(b), geo.block_end(b + m - 1)
        pieces, f = [], f_lo
        while f < f_hi:
            k = f_hi - f if piece is None else min(f_hi - f, piece)
            pieces.append((f, k, f != f_lo))
            f += k
        ranges.append((b, m, pieces))
        b += m
    return ranges, (slots, per, carried)
