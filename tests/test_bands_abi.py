"""sgx_bands_batch / sgx_bands_fused (PCM to the log-frequency rows' magnitude_in means) through every layer, without a GPU:
the C header, the exports of libsgx.so, the ctypes table, the engine and the Rust binding."""
import ctypes
import os
import re

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_bands_batch", "sgx_bands_fused")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_bands():
    h = _read("include", "sgx.h")
    for name in NEW:
        assert re.search(rf"SGX_API\s+int\s+{name}\s*\(", h), name
    assert re.search(r"#define\s+SGX_LIVE_BANDS\s+3\b", h)


def test_library_exports_bands():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_bindings():
    assert _lib.LIVE_BANDS == 3
    names = {s[0] for s in _lib.SIGNATURES}
    assert set(NEW) <= names
    assert callable(getattr(SpectrogramEngine, "bands_batch", None))
    assert isinstance(SpectrogramEngine.__dict__.get("bands_fused"), property)


def test_rust_binding():
    rs = _read("bindings", "rust", "sgx_sys.rs")
    for name in NEW:
        assert re.search(rf"pub fn {name}\s*\(", rs), name
    assert re.search(r"pub const SGX_LIVE_BANDS: c_int = 3;", rs)
