"""sgx_bands_peak_batch / sgx_bands_peak_fused / sgx_render_bands (peak-hold band columns over groups of frames, and the colour of a
band column) through every layer, without a GPU: the C header, the exports of libsgx.so, the ctypes table, the engine, the C++ mirror
and the Rust binding."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_bands_peak_batch", "sgx_bands_peak_fused", "sgx_render_bands")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_peak():
    h = _read("include", "sgx.h")
    for name in NEW:
        assert re.search(rf"SGX_API\s+int\s+{name}\s*\(", h), name
    # the group sits between max_frames and the output, as a size_t
    assert re.search(r"sgx_bands_peak_batch\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*size_t first_frame,\s*"
                     r"size_t max_frames,\s*size_t group,\s*float\s*\*d_peak,\s*size_t\s*\*n_out\)", h)
    assert re.search(r"sgx_render_bands\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_bands,\s*size_t n_columns,\s*uint8_t\s*\*d_rgba\)", h)
    # the conventions list names the family among the calls that only enqueue
    assert "sgx_bands_*batch" in h.split("Conventions")[1].split("*/")[0]


def test_library_exports_peak():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig)
    assert len(sig["sgx_bands_peak_batch"][2]) == 8 and sig["sgx_bands_peak_batch"][2][5] is ctypes.c_size_t
    assert len(sig["sgx_render_bands"][2]) == 4
    assert len(sig["sgx_bands_peak_fused"][2]) == 1
    params = list(inspect.signature(SpectrogramEngine.bands_peak_batch).parameters)
    assert params == ["self", "pcm", "group", "first_frame", "max_frames", "out"]
    assert list(inspect.signature(SpectrogramEngine.render_bands).parameters) == ["self", "bands", "out"]
    assert isinstance(SpectrogramEngine.__dict__.get("bands_peak_fused"), property)


def test_cpp_mirror_and_rust_binding():
    assert "sgx_bands_peak_batch(" in _read("include", "sgx.hpp")
    rs = _read("bindings", "rust", "sgx_sys.rs")
    for name in NEW:
        assert re.search(rf"pub fn {name}\s*\(", rs), name
    assert re.search(r"pub fn sgx_bands_peak_batch\([^)]*group: usize,\s*d_peak: \*mut f32,\s*n_out: \*mut usize\)", rs)


def test_documents_name_the_calls():
    assert "sgx_bands_peak_batch" in _read("README.md")
    assert "sgx_bands_peak_batch" in _read("DESIGN.md") and "sgx_render_bands" in _read("DESIGN.md")
    assert "sgx_bands_peak_batch" in _read("INTEGRATION.md")
