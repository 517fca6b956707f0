"""sgx_mel_weights through ctypes, without a GPU: the triangular mel bank over the true bin frequencies k * sample_rate / (2 W),
scattered to a dense [n_mels][M] matrix, against the same formulas in numpy float64 (include/sgx.h states them).  Tolerance:
|delta| <= 2^-23 |w| + 1e-12 -- the one rounding to float, plus a last-bit difference between libm and numpy in the mel points ahead of
it.  Dense matrices are compared, not first / count: a bin that sits on a filter's edge may be in or out."""
import ctypes as C

import numpy as np
import pytest

from spectrogram_rs_amd import _lib, mel_weights

CASES = [(48000.0, 2048, 128, 0.0, 24000.0), (48000.0, 2048, 80, 32.0, 22030.0), (16000.0, 400, 80, 0.0, 8000.0),
         (48000.0, 2048, 256, 20.0, 20000.0), (48000.0, 64, 40, 0.0, 24000.0)]


def hz_to_mel(f, scale):
    f = np.asarray(f, np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m, scale):
    m = np.asarray(m, np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def reference(sr, W, n_mels, f_min, f_max, scale, norm):
    pts = mel_to_hz(np.linspace(hz_to_mel(f_min, scale), hz_to_mel(f_max, scale), n_mels + 2), scale)
    f = np.arange(1, W) * sr / (2.0 * W)                       # stored element j is bin k = j + 1
    lo, c, hi = pts[:-2, None], pts[1:-1, None], pts[2:, None]
    w = np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)))
    return w * (2.0 / (hi - lo)) if norm == "slaney" else w


def scatter(first, count, weights, M):
    d = np.zeros((len(first), M))
    off = 0
    for m in range(len(first)):
        assert first[m] + count[m] <= M
        d[m, first[m]:first[m] + count[m]] = weights[off:off + count[m]]
        off += count[m]
    assert off == len(weights)
    return d


@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("scale", ["htk", "slaney"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "sr%d_w%d_m%d" % (c[0], c[1], c[2]))
def test_mel_weights_against_numpy(case, scale, norm):
    sr, W, n_mels, f_min, f_max = case
    first, count, weights = mel_weights(sr, W, n_mels, f_min, f_max, scale, norm)
    assert first.dtype == np.uint32 and count.dtype == np.uint32 and weights.dtype == np.float32
    assert len(first) == len(count) == n_mels and weights.size == count.sum()
    got, ref = scatter(first, count, weights, W - 1), reference(sr, W, n_mels, f_min, f_max, scale, norm)
    assert (np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-12).all(), float(np.abs(got - ref).max())
    assert (weights > 0).all()                                  # the support is the bins with w > 0
    # filters narrower than the bin spacing with no bin inside come out empty: none but at W 64, where numpy counts six on the HTK
    # scale (seven on Slaney's)
    assert np.array_equal(count == 0, ref.max(axis=1) == 0)
    assert int((count == 0).sum()) == (0 if W != 64 else 6 if scale == "htk" else 7)


def test_sizing_call_and_invalid_arguments():
    lib = _lib.load()
    n = C.c_size_t(99)
    args = (C.c_double(48000.0), 2048, 128, C.c_double(0.0), C.c_double(24000.0), _lib.MEL_HTK, _lib.MEL_NORM_NONE)
    assert lib.sgx_mel_weights(*args, None, None, None, C.byref(n)) == 0
    first, count, weights = mel_weights(48000.0, 2048, 128)
    assert n.value == weights.size == count.sum() and 3500 < n.value < 4500
    bad = _lib.SGX_ERR_INVALID_ARG

    def call(sr=48000.0, W=2048, mels=128, lo=0.0, hi=24000.0, scale=0, norm=0):
        return lib.sgx_mel_weights(C.c_double(sr), W, mels, C.c_double(lo), C.c_double(hi), scale, norm, None, None, None, C.byref(n))

    assert call() == 0
    for kw in (dict(mels=0), dict(lo=-1.0), dict(lo=100.0, hi=100.0), dict(lo=200.0, hi=100.0), dict(hi=24000.5), dict(W=1), dict(W=0),
               dict(scale=2), dict(norm=2), dict(sr=0.0)):
        assert call(**kw) == bad, kw
        assert n.value == 0
    assert lib.sgx_mel_weights(*args, None, None, None, None) == bad
    f = np.zeros(128, np.uint32)
    assert lib.sgx_mel_weights(*args, f.ctypes.data_as(C.c_void_p), None, None, C.byref(n)) == bad      # only some of the arrays
    assert call(hi=24000.0) == 0 and call(sr=44100.0, hi=22050.0) == 0                                   # f_max = sample_rate / 2 is allowed
