"""tests/fbank_reference.py, without a GPU: the host reference of the filterbank sums' definition (include/sgx.h) is held to libm's fmaf,
to a scalar loop written straight from the header, and to the properties the GPU tests rely on -- its inputs tell sum orders apart, its
bank has the stated edges, and no intermediate on the GPU tests' synthetic rows is denormal (so the device's denormal mode, which the
header does not state, plays no part in tests/test_gpu_fbank_order.py)."""
import ctypes as C

import numpy as np
import pytest

import fbank_reference as fr
from spectrogram_rs_amd import mel_weights

libm = C.CDLL("libm.so.6")
libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
libm.fmaf.restype = C.c_float


def fmaf(w, x, a):
    return np.float32(libm.fmaf(float(w), float(x), float(a)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- fma32 ----------------------------------------------------------------------------------------------------------------------------
def triples(n, seed):
    """both signs, 14 binades; one third of the addends nearly cancel the product, where a double rounding shows most"""
    rng = np.random.default_rng(seed)
    v = lambda: (np.exp2(rng.uniform(-7.0, 7.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    w, x, a = v(), v(), v()
    near = rng.random(n) < 1.0 / 3.0
    cancel = (-(w * x) * (1.0 + rng.integers(-4, 5, n) * 2.0 ** -23)).astype(np.float32)
    return w, x, np.where(near, cancel, a)


def test_fma32_equals_libm_fmaf():
    w, x, a = triples(120_000, 7)
    got = fr.fma32(w, x, a)
    want = np.array([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(w, x, a)], np.float32)
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {w.size} triples differ from fmaf"
    # the signs of zero: a product of -0 into the chain's +0 is +0, and -0 + -0 stays -0
    for p, q, r in [(-1.0, 0.0, 0.0), (1.0, 0.0, -0.0), (-1.0, 0.0, -0.0), (0.0, 0.0, 0.0), (1.0, 1.0, -1.0)]:
        assert bits(fr.fma32(p, q, r)) == bits(fmaf(p, q, r)), (p, q, r)


def double_rounding_cases():
    """w x lies exactly halfway between two float32 and the addend is far below the float64 sum's last bit: only its sign decides"""
    w, x, a = [], [], []
    for e in range(-5, 6):
        for sw in (1.0, -1.0):
            for sa in (1.0, -1.0):
                w.append(sw * (1.0 + 2.0 ** -12))
                x.append((1.0 + 2.0 ** -12) * 2.0 ** e)
                a.append(sa * 2.0 ** (e - 60))
    return np.array(w, np.float32), np.array(x, np.float32), np.array(a, np.float32)


def test_fma32_on_double_rounding_cases():
    w, x, a = double_rounding_cases()
    want = np.array([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(w, x, a)], np.float32)
    assert np.array_equal(bits(fr.fma32(w, x, a)), bits(want))
    naive = (w.astype(np.float64) * x.astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    wrong = int((bits(naive) != bits(want)).sum())
    assert wrong >= 1, "the float64-then-cast formula passes these cases: they do not bite"
    assert wrong == w.size // 2                            # the half whose addend pulls away from the even neighbour


# ---- bank_sums and cross_sums against a scalar loop from the header ----------------------------------------------------------------
def scalar_sums(x, bank):
    """x [M][C] float32 -> [n_filters][C]: include/sgx.h, one element at a time"""
    first, count, weights = bank
    out = np.zeros((len(first), x.shape[1]), np.float32)
    off = 0
    for f in range(len(first)):
        for c in range(x.shape[1]):
            a = [np.float32(0.0)] * 64
            for i in range(int(count[f])):
                a[i % 64] = fmaf(weights[off + i], x[int(first[f]) + i, c], a[i % 64])
            for s in (32, 16, 8, 4, 2, 1):
                for l in range(s):
                    a[l] = np.float32(a[l] + a[l + s])
            out[f, c] = a[0]
        off += int(count[f])
    return out


def small_bank(M, seed):
    rng = np.random.default_rng(seed)
    first, count, weights = [], [], []
    for n in rng.permutation([0, 1, 64, 65, 200]):
        first.append(int(rng.integers(0, M - n + 1)))
        count.append(int(n))
        weights.append((np.exp2(rng.uniform(-6.0, 0.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32))
    return np.array(first, np.uint32), np.array(count, np.uint32), np.concatenate(weights)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sums_equal_the_scalar_loop(seed):
    M = 256
    bank = small_bank(M, seed)
    rows = fr.synthetic_mags(1, M, seed)[0]
    for power in (1, 2):
        x = rows if power == 1 else np.array([[np.float32(v * v) for v in r] for r in rows], np.float32)
        assert np.array_equal(bits(fr.bank_sums(rows, bank, power)), bits(scalar_sums(x, bank))), f"power {power}"
    spec = fr.synthetic_spec(1, M, seed)[0]
    x = np.zeros((M, 4), np.float32)
    for j in range(M):
        (a, b), (c, d) = spec[j]
        x[j] = [np.float32(np.float32(a * a) + np.float32(b * b)), np.float32(np.float32(c * c) + np.float32(d * d)),
                np.float32(np.float32(a * c) + np.float32(b * d)), np.float32(np.float32(b * c) - np.float32(a * d))]
    got = fr.cross_sums(spec, bank)
    assert np.array_equal(bits(got), bits(scalar_sums(x, bank)))
    empty = bank[1] == 0
    assert empty.any() and (bits(got[empty]) == 0).all() and (bits(fr.bank_sums(rows, bank, 2)[empty]) == 0).all()
    # the batched form is the per-column form
    cols = fr.synthetic_mags(3, M, seed + 10)
    assert np.array_equal(bits(fr.bank_sums(cols, bank, 2)), bits(np.stack([fr.bank_sums(c, bank, 2) for c in cols])))


def test_filter_levels_end_in_the_sum():
    M = 300
    bank = small_bank(M, 4)
    x = fr.elements(fr.synthetic_mags(2, M, 4), 2)
    want = fr.bank_sums(fr.synthetic_mags(2, M, 4), bank, 2)
    for f in range(len(bank[0])):
        if bank[1][f]:
            levels = fr.filter_levels(x, bank, f)
            assert [v.shape[-2] for v in levels] == [64, 32, 16, 8, 4, 2, 1]
            assert np.array_equal(bits(levels[-1][..., 0, :]), bits(want[..., f, :]))


# ---- the inputs of the GPU tests tell sum orders apart --------------------------------------------------------------------------------
M_ORDER = 2047
SR = 48000.0


def order_banks(W):
    return {"edges": fr.edge_bank(W - 1), "mel128": mel_weights(SR, W, 128, 0.0, SR / 2)}


@pytest.mark.parametrize("kind", ["edges", "mel128"])
def test_inputs_tell_orders_apart(kind):
    bank = order_banks(M_ORDER + 1)[kind]
    long_enough = bank[1] >= 3
    for x, what in [(fr.elements(fr.synthetic_mags(3, M_ORDER, 101), 1), "power 1"), (fr.elements(fr.synthetic_mags(3, M_ORDER, 101), 2), "power 2"),
                    (fr.cross_elements(fr.synthetic_spec(3, M_ORDER, 102)), "cross")]:
        ref = fr._sums(x, bank)
        left = fr.mutant_sums(x, bank, tree="left")
        stride32 = fr.mutant_sums(x, bank, stride=32)
        d_left = (bits(ref) != bits(left)).any(axis=(0, 2))
        d_stride = (bits(ref) != bits(stride32)).any(axis=(0, 2))
        assert d_left.any(), f"{kind}/{what}: a left-to-right sum of the 64 partial sums gives the same bits"
        assert d_stride.any(), f"{kind}/{what}: chains of lane stride 32 give the same bits"
        assert not d_left[~long_enough].any()              # (one or two terms: any order is the same sum)
        assert not d_stride[bank[1] <= 32].any()            # (no lane has a second element: the stride plays no part)
        # several filters see it, not one lucky one
        print(f"{kind}/{what}: another tree shows in {int(d_left.sum())} of {int(long_enough.sum())} filters, another stride in {int(d_stride.sum())} of {int((bank[1] > 32).sum())}")
        assert d_left.sum() >= 8 and d_stride.sum() >= 8
        # a sum that lands on another filter's place is seen as well: the non-empty filters' outputs are all different
        flat = bits(ref).transpose(1, 0, 2).reshape(ref.shape[1], -1)
        nonempty = np.flatnonzero(bank[1] > 0)
        assert len({tuple(r) for r in flat[nonempty]}) == len(nonempty), f"{kind}/{what}: two filters give the same bits"


# ---- edge_bank ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [22, 63, 255, 2047, 8191, 2 ** 20 - 1])
def test_edge_bank(M):
    first, count, weights = fr.edge_bank(M)
    again = fr.edge_bank(M)
    assert all(np.array_equal(u, v) for u, v in zip((first, count, weights), again)), "not deterministic"
    assert first.dtype == np.uint32 and count.dtype == np.uint32 and weights.dtype == np.float32
    assert len(first) == len(count) == fr.N_EDGE_FILTERS == 263
    assert sorted((263 - w + 3) // 4 for w in range(4)) == [65, 66, 66, 66]       # per wave of a 4-wave pass: 64 parked results, then 2 or 1
    f64, c64 = first.astype(np.int64), count.astype(np.int64)
    assert (f64 + c64 <= M).all() and weights.size == c64.sum()
    assert (np.diff(f64) < 0).any() and (np.diff(f64) > 0).any(), "the filters are in ascending order"
    assert not np.array_equal(np.lexsort((c64, f64)), np.arange(263))
    mag = np.abs(weights)
    assert (mag >= 2.0 ** -6).all() and (mag <= 1.0).all() and (weights < 0).any() and (weights > 0).any()
    have = set(zip(f64.tolist(), c64.tolist()))
    assert {(0, 1), (M - 1, 1), (M, 0), (0, 0), (0, M)} <= have
    off = fr._offsets(count)
    whole = [f for f in range(263) if f64[f] == 0 and c64[f] == M and M > 129]
    if M > 129:
        assert len(whole) == 1
        w = weights[off[whole[0]]:off[whole[0] + 1]]
        assert (np.sign(w[::2]) == np.sign(w[0])).all() and (np.sign(w[1::2]) == -np.sign(w[0])).all()
    else:
        assert any((np.sign(weights[off[f]:off[f + 1]][1:]) == -np.sign(weights[off[f]:off[f + 1]][:-1])).all()
                   for f in range(263) if f64[f] == 0 and c64[f] == M)
    for n in fr.EDGE_COUNTS:
        n = min(n, M)
        assert (0, n) in have and (M - n, n) in have, f"count {n}: not at both ends"
    assert fr.EDGE_COUNTS == (2, 63, 64, 65, 127, 128, 129)
    singles = int((c64 == 1).sum())
    assert singles >= 263 - 5 - 2 * len(fr.EDGE_COUNTS) + 2
    if M == 2047:
        assert 3000 <= weights.size <= 4000 and weights.size <= 16384 and 263 <= 1024      # within the fused limit (include/sgx.h: sgx_fbank_fused)
    assert not np.array_equal(fr.edge_bank(M, seed=1)[2], weights), "the seed plays no part"


# ---- no denormal anywhere on the GPU tests' rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 2048, 2400])
def test_no_intermediate_is_denormal(W):
    M = W - 1
    seen = []

    def watch(a):
        seen.append(a.size)
        assert fr.zero_or_normal(a), "an intermediate of the reference is denormal or not finite"

    for kind, bank in order_banks(W).items():
        for power in (1, 2):
            fr.bank_sums(fr.synthetic_mags(3, M, 101), bank, power, watch)
        fr.cross_sums(fr.synthetic_spec(3, M, 102), bank, watch)
    assert len(seen) > 1000
    assert not fr.zero_or_normal(np.array([1e-40], np.float32)) and not fr.zero_or_normal(np.array([np.inf], np.float32))
    assert fr.zero_or_normal(np.array([0.0, -0.0, 2.0 ** -126, -3.0e38], np.float32))


def test_stage_decisions_restate_the_launchers():
    """launch_fbank_stage: M * sizeof(float2) <= min(lds_optin, 160 KiB); launch_fbank_cross_stage: M * 2 * sizeof(float2)"""
    import os

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spectrogram_rs_amd", "csrc", "sgx_fbank.hip")).read()
    for text in ("(size_t)c->M * sizeof(float2) <= lds_cap", "(size_t)c->M * 2 * sizeof(float2) <= lds_cap", "(size_t)160 * 1024"):
        assert text in src, text
    assert fr.stage_staged(20480) and not fr.stage_staged(20481)               # W 20481 | 20482
    assert fr.cross_stage_staged(10240) and not fr.cross_stage_staged(10241)   # W 10241 | 10242
    assert not fr.stage_staged(20480, 64 * 1024) and fr.stage_staged(8192, 64 * 1024)
