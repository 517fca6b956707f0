"""sgx_stft_batch_complex (the complex (L, R) spectra behind sgx_stft_batch's magnitudes) through every layer, without a GPU: the C header,
the exports of libsgx.so, the ctypes table, the engine, the C++ mirror and the Rust binding."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sgx_stft_batch_complex"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_complex_rows():
    h = _read("include", "sgx.h")
    m = re.search(rf"SGX_API\s+int\s+{NAME}\s*\(([^;]*)\);", h)
    assert m, NAME
    assert re.sub(r"\s+", " ", m.group(1)) == ("sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame, "
                                               "size_t max_frames, float *d_spec, size_t *n_out")
    assert "d_spec [n_out][pairs][M][2][2] float" in h


def test_library_exports_complex_rows():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    assert hasattr(lib, NAME)


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert NAME in sig
    assert sig[NAME][2] == sig["sgx_stft_batch"][2]
    fn = getattr(SpectrogramEngine, "stft_batch_complex", None)
    assert callable(fn)
    assert list(inspect.signature(fn).parameters) == ["self", "pcm", "first_frame", "max_frames", "out"]


def test_cpp_mirror():
    assert re.search(rf"\b{NAME}\s*\(", _read("include", "sgx.hpp"))


def test_rust_binding():
    assert re.search(rf"pub fn {NAME}\s*\(", _read("bindings", "rust", "sgx_sys.rs"))
