"""sgx_istft_batch (PCM from the complex (L, R) spectra of sgx_stft_batch_complex) through every layer, without a GPU: the C header,
the exports of libsgx.so, the ctypes table, the engine, the C++ mirror, the Rust binding and INTEGRATION.md."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sgx_istft_batch", "sgx_istft_supported")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_inverse():
    h = _read("include", "sgx.h")
    m = re.search(r"SGX_API\s+int\s+sgx_istft_batch\s*\(([^;]*)\);", h)
    assert m
    assert re.sub(r"\s+", " ", m.group(1)) == ("sgx_ctx *ctx, const float *d_spec, size_t n_frames, size_t first_sample, "
                                               "size_t max_samples, float *d_pcm, size_t *n_out")
    m = re.search(r"SGX_API\s+int\s+sgx_istft_supported\s*\(([^;]*)\);", h)
    assert m and re.sub(r"\s+", " ", m.group(1)) == "const sgx_ctx *ctx"
    assert "g = W * ifft(A).real" in h and "f0 * H + n" in h


def test_library_exports_the_inverse():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for n in NAMES:
        assert hasattr(lib, n), n


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert sig["sgx_istft_batch"][1:] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                         ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)])
    assert sig["sgx_istft_supported"][1:] == (ctypes.c_int, [ctypes.c_void_p])
    fn = getattr(SpectrogramEngine, "istft_batch", None)
    assert callable(fn)
    assert list(inspect.signature(fn).parameters) == ["self", "spec", "first_sample", "max_samples", "out"]
    assert list(inspect.signature(SpectrogramEngine.istft_supported).parameters) == ["self"]


def test_cpp_mirror():
    hpp = _read("include", "sgx.hpp")
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", hpp), n


def test_rust_binding():
    rs = _read("bindings", "rust", "sgx_sys.rs")
    for n in NAMES:
        assert re.search(rf"pub fn {n}\s*\(", rs), n
    assert "pub fn sgx_istft_batch" in _read("INTEGRATION.md")


def test_integration_is_in_sync():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sync_integration.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
