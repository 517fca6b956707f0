"""The filterbank sums of include/sgx.h on the host, bit for bit: written from the header's text alone, in numpy, with no GPU and no torch.

The header defines the output of sgx_fbank_batch / sgx_fbank_mags and of sgx_fbank_cross_batch / sgx_fbank_cross_spec down to the bit:
  x = m (power 1) or rn(m * m) (power 2); for the cross sums the four products of a bin, every product rounded, then one add or subtract;
  1. 64 partial sums: a[l] takes the elements i = l, l + 64, ... in ascending order as one chain of fused multiply-adds from +0;
  2. a tree by halving: for s = 32, 16, 8, 4, 2, 1 in turn a[l] = a[l] + a[l + s] for every l < s; the sum is a[0].
An empty filter gives +0.0.

numpy has no fused multiply-add.  fma32 builds one from float64: the product of two float32 is exact in float64 (24 x 24 bits), the
addition is taken apart by TwoSum, and where its error term is not zero the float64 sum is rounded to odd before the cast to float32.
Rounding to odd at 53 bits and then to nearest at 24 is a single correct rounding (the sticky bit survives the first step);
tests/test_fbank_reference.py holds it to libm's fmaf.

bank_sums and cross_sums take an optional `watch`, called with every intermediate array (the products, every state of the chains, every
level of the tree), and filter_levels returns one filter's partial sums per level: what a disagreement with the device is reported by."""
import numpy as np

LANES = 64
LEVELS = (32, 16, 8, 4, 2, 1)
N_EDGE_FILTERS = 263           # 4 waves: 66, 66, 66 and 65 filters -- one full flush of 64 parked results, then a ragged group of 2 or 1
EDGE_COUNTS = (2, 63, 64, 65, 127, 128, 129)


def fma32(w, x, a):
    """rn(w * x + a) in float32 with a single rounding, elementwise"""
    w, x, a = (np.asarray(v, np.float32).astype(np.float64) for v in (w, x, a))
    p = w * x                                              # exact
    s = p + a
    bb = s - p                                             # TwoSum (Knuth): s + e == p + a exactly
    e = (p - (s - bb)) + (a - bb)
    even = (np.atleast_1d(s).view(np.int64) & 1) == 0
    toward = np.where(e > 0.0, np.inf, -np.inf)
    s = np.where((e != 0.0) & even.reshape(np.shape(s)), np.nextafter(s, toward), s)      # inexact: the neighbour with the odd last bit
    return s.astype(np.float32)


def _offsets(count):
    return np.concatenate([[0], np.cumsum(np.asarray(count, np.int64))])


def _chains(x, w, watch=None, stride=LANES):
    """x [..., count, C] float32, w [count] -> the partial sums a [..., stride, C]: a[l] = the fma chain over i = l, l + stride, ... from +0"""
    count = w.shape[0]
    a = np.zeros(x.shape[:-2] + (stride, x.shape[-1]), np.float32)
    for start in range(0, count, stride):
        n = min(stride, count - start)
        a[..., :n, :] = fma32(w[start:start + n, None], x[..., start:start + n, :], a[..., :n, :])
        if watch is not None:
            watch(a)
    return a


def _tree(a, watch=None):
    """the levels of the halving tree over a [..., 64, C]: a list of 6 arrays, the last [..., 1, C]"""
    out = []
    for s in LEVELS:
        a = (a[..., :s, :] + a[..., s:2 * s, :]).astype(np.float32)
        if watch is not None:
            watch(a)
        out.append(a)
    return out


def _sums(x, bank, watch=None):
    """x [..., M, C] float32 -> [..., n_filters, C] float32 in the header's order"""
    first, count, weights = bank
    weights = np.asarray(weights, np.float32)
    off = _offsets(count)
    out = np.zeros(x.shape[:-2] + (len(first), x.shape[-1]), np.float32)
    for f in range(len(first)):
        c, j = int(count[f]), int(first[f])
        if c == 0:
            continue                                       # exactly +0.0
        a = _chains(x[..., j:j + c, :], weights[off[f]:off[f + 1]], watch)
        out[..., f, :] = _tree(a, watch)[-1][..., 0, :]
    return out


def elements(rows, power):
    """x of the magnitude sums: m, or m * m rounded to float32"""
    m = np.asarray(rows, np.float32)
    assert power in (1, 2)
    return m if power == 1 else (m * m).astype(np.float32)


def cross_elements(spec):
    """x0 .. x3 of the cross sums: [..., M, 2, 2] float32 (L.re, L.im), (R.re, R.im) -> [..., M, 4], products rounded, then one add or subtract"""
    s = np.asarray(spec, np.float32)
    a, b, c, d = s[..., 0, 0], s[..., 0, 1], s[..., 1, 0], s[..., 1, 1]
    mul = lambda u, v: (u * v).astype(np.float32)
    return np.stack([(mul(a, a) + mul(b, b)).astype(np.float32), (mul(c, c) + mul(d, d)).astype(np.float32),
                     (mul(a, c) + mul(b, d)).astype(np.float32), (mul(b, c) - mul(a, d)).astype(np.float32)], -1)


def bank_sums(rows, bank, power, watch=None):
    """rows [..., M, 2] float32 (what sgx_stft_batch stores) -> [..., n_filters, 2] float32: sgx_fbank_mags to the bit"""
    x = elements(rows, power)
    if watch is not None:
        watch(x)
    return _sums(x, bank, watch)


def cross_sums(spec, bank, watch=None):
    """spec [..., M, 2, 2] float32 (what sgx_stft_batch_complex stores) -> [..., n_filters, 4] float32: sgx_fbank_cross_spec to the bit"""
    x = cross_elements(spec)
    if watch is not None:
        watch(x)
    return _sums(x, bank, watch)


def filter_levels(x, bank, f):
    """filter f over the elements x [..., M, C]: [the 64 chains, then the tree's six levels] -- for reporting the first partial sum that differs"""
    first, count, weights = bank
    off = _offsets(count)
    c, j = int(count[f]), int(first[f])
    a = _chains(x[..., j:j + c, :], np.asarray(weights, np.float32)[off[f]:off[f + 1]])
    return [a] + _tree(a)


def zero_or_normal(a):
    """every float32 of a is +-0 or has a normal exponent (no denormal, infinity or NaN)"""
    e = (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 23) & 0xFF
    mant = np.ascontiguousarray(a, np.float32).view(np.uint32) & 0x7FFFFF
    return bool((((e > 0) & (e < 255)) | ((e == 0) & (mant == 0))).all())


# ---- mutants: the orders a faulty kernel could take, for showing that a test's inputs tell them apart ----------------------------------
def mutant_sums(x, bank, tree="halving", stride=LANES):
    """_sums with another tree ("left": a[0] + a[1] + ... left to right) or another lane stride (the chains of `stride` lanes, the missing
    lanes of the tree zero)"""
    first, count, weights = bank
    weights = np.asarray(weights, np.float32)
    off = _offsets(count)
    out = np.zeros(x.shape[:-2] + (len(first), x.shape[-1]), np.float32)
    for f in range(len(first)):
        c, j = int(count[f]), int(first[f])
        if c == 0:
            continue
        a = _chains(x[..., j:j + c, :], weights[off[f]:off[f + 1]], None, stride)
        if stride < LANES:
            a = np.concatenate([a, np.zeros(a.shape[:-2] + (LANES - stride, a.shape[-1]), np.float32)], -2)
        if tree == "left":
            s = a[..., 0, :]
            for l in range(1, LANES):
                s = (s + a[..., l, :]).astype(np.float32)
            out[..., f, :] = s
        else:
            out[..., f, :] = _tree(a)[-1][..., 0, :]
    return out


# ---- the bank and the rows of the order tests ---------------------------------------------------------------------------------------
def edge_bank(M, seed=0):
    """(first, count, weights) of 263 filters over M bins, in a seeded shuffled order: bin 0 alone, bin M - 1 alone, the empty filters
    (M, 0) and (0, 0), the whole spectrum with alternating signs, filters of 2, 63, 64, 65, 127, 128 and 129 bins (clipped to M) once
    from bin 0 and once ending at bin M, and single bins at seeded places for the rest.  Weights of both signs, magnitudes in [2^-6, 1]."""
    assert M >= 1
    rng = np.random.default_rng([0xFBA2C, int(M), int(seed)])

    def w(n, alternate=False):
        mag = np.exp2(rng.uniform(-6.0, 0.0, n))
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) if alternate else rng.choice([-1.0, 1.0], n)
        return (mag * sign).astype(np.float32)

    filters = [(0, w(1)), (M - 1, w(1)), (M, w(0)), (0, w(0)), (0, w(M, alternate=True))]
    for n in EDGE_COUNTS:
        n = min(n, M)
        filters += [(0, w(n)), (M - n, w(n))]
    while len(filters) < N_EDGE_FILTERS:
        filters.append((int(rng.integers(0, M)), w(1)))
    order = rng.permutation(len(filters))
    filters = [filters[i] for i in order]
    first = np.array([f for f, _ in filters], np.uint32)
    count = np.array([len(v) for _, v in filters], np.uint32)
    return first, count, np.concatenate([v for _, v in filters]).astype(np.float32)


def synthetic_mags(columns, M, seed):
    """[columns][M][2] float32 magnitudes 2^U(-10, 0): normal range, and so are their squares"""
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(-10.0, 0.0, (columns, M, 2))).astype(np.float32)


def synthetic_spec(columns, M, seed):
    """[columns][M][2][2] float32 complex rows, magnitudes 2^U(-10, 0) of either sign"""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.uniform(-10.0, 0.0, (columns, M, 2, 2)))
    return (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)


# ---- which body the stage kernels run (launch_fbank_stage, launch_fbank_cross_stage: the column in LDS, or read where it lies) ---------
STAGE_LDS_CAP = 160 * 1024


def stage_staged(M, lds_optin=STAGE_LDS_CAP):
    return M * 8 <= min(lds_optin, STAGE_LDS_CAP)


def cross_stage_staged(M, lds_optin=STAGE_LDS_CAP):
    return M * 16 <= min(lds_optin, STAGE_LDS_CAP)
