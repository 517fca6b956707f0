"""sgx_fbank_* and sgx_mel_weights (a filterbank over the bin magnitudes or powers, PCM to mel and filterbank energies) through every
layer, without a GPU: the C header, the exports of libsgx.so, the ctypes table, the engine and FilterBank, the C++ mirror, the Rust
binding and the documents."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import FilterBank, SpectrogramEngine, _lib, mel_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_fbank_create", "sgx_fbank_destroy", "sgx_fbank_filters", "sgx_fbank_batch", "sgx_fbank_mags", "sgx_fbank_fused", "sgx_mel_weights")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_filterbank_calls():
    h = _read("include", "sgx.h")
    assert "typedef struct sgx_fbank sgx_fbank;" in h
    for name in NEW:
        assert re.search(rf"SGX_API\s+(int|void|uint32_t)\s+{name}\s*\(", h), name
    assert re.search(r"SGX_API\s+int\s+sgx_fbank_create\s*\(\s*sgx_ctx\s*\*ctx,\s*uint32_t n_filters,\s*const uint32_t\s*\*h_first,\s*"
                     r"const uint32_t\s*\*h_count,\s*const float\s*\*h_weights,\s*uint32_t power,\s*void\s*\*\*out_fbank\)", h)
    assert re.search(r"SGX_API\s+int\s+sgx_fbank_batch\s*\(\s*void\s*\*fbank,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*size_t first_frame,\s*"
                     r"size_t max_frames,\s*float\s*\*d_out,\s*size_t\s*\*n_out\)", h)
    assert re.search(r"SGX_API\s+int\s+sgx_fbank_mags\s*\(\s*void\s*\*fbank,\s*const float\s*\*d_mags,\s*size_t n_columns,\s*float\s*\*d_out\)", h)
    assert re.search(r"SGX_API\s+int\s+sgx_mel_weights\s*\(\s*double sample_rate,\s*uint32_t window_samples,\s*uint32_t n_mels,\s*double f_min,\s*"
                     r"double f_max,\s*uint32_t scale,\s*uint32_t norm,\s*uint32_t\s*\*h_first,\s*uint32_t\s*\*h_count,\s*float\s*\*h_weights,\s*"
                     r"size_t\s*\*n_weights\)", h)
    for name, value in (("SGX_MEL_HTK", 0), ("SGX_MEL_SLANEY", 1), ("SGX_MEL_NORM_NONE", 0), ("SGX_MEL_NORM_SLANEY", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}u\b", h), name
    # the conventions list names the two calls among those that only enqueue
    conventions = h.split("Conventions")[1].split("*/")[0]
    assert "sgx_fbank_batch" in conventions and "sgx_fbank_mags" in conventions
    # the definition: the sum's order, the limits of the fused route, the axis of the mel bank
    for words in ("balanced binary tree", "fused multiply-add", "exactly +0.0f", "1024 filters", "16384 weights", "quirk Q2", "ln(6.4) / 27"):
        assert words in re.sub(r"\s*\n \*\s*", " ", h), words


def test_library_exports_the_filterbank_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig)
    assert len(sig["sgx_fbank_create"][2]) == 7 and sig["sgx_fbank_create"][2][1] is ctypes.c_uint32
    assert len(sig["sgx_fbank_batch"][2]) == 7 and sig["sgx_fbank_batch"][2][2] is ctypes.c_size_t
    assert len(sig["sgx_fbank_mags"][2]) == 4 and len(sig["sgx_fbank_fused"][2]) == 1 and len(sig["sgx_fbank_filters"][2]) == 1
    assert sig["sgx_fbank_filters"][1] is ctypes.c_uint32 and sig["sgx_fbank_destroy"][1] is None
    assert len(sig["sgx_mel_weights"][2]) == 11 and sig["sgx_mel_weights"][2][0] is ctypes.c_double
    assert (_lib.MEL_HTK, _lib.MEL_SLANEY, _lib.MEL_NORM_NONE, _lib.MEL_NORM_SLANEY) == (0, 1, 0, 1)
    assert list(inspect.signature(SpectrogramEngine.filterbank).parameters) == ["self", "first", "count", "weights", "power"]
    assert inspect.signature(SpectrogramEngine.filterbank).parameters["power"].default == 2
    mel = inspect.signature(SpectrogramEngine.mel_filterbank).parameters
    assert list(mel) == ["self", "n_mels", "f_min", "f_max", "scale", "norm", "power"]
    assert [mel[k].default for k in list(mel)[1:]] == [128, 0.0, None, "htk", None, 2]
    assert list(inspect.signature(FilterBank.batch).parameters) == ["self", "pcm", "first_frame", "max_frames", "out"]
    assert list(inspect.signature(FilterBank.apply).parameters) == ["self", "mags", "out"]
    assert isinstance(FilterBank.__dict__.get("fused"), property) and isinstance(FilterBank.__dict__.get("n_filters"), property)
    assert callable(FilterBank.close)
    assert list(inspect.signature(mel_weights).parameters) == ["sample_rate", "window_samples", "n_mels", "f_min", "f_max", "scale", "norm"]
    # closed by the engine like the rings
    assert "_rings" in inspect.getsource(SpectrogramEngine.filterbank) and "use_current_stream" in inspect.getsource(SpectrogramEngine._out)


def test_cpp_mirror_and_rust_binding():
    hpp = _read("include", "sgx.hpp")
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hpp), name
    assert "class FilterBank" in hpp
    rs = _read("bindings", "rust", "sgx_sys.rs")
    for name in NEW:
        assert re.search(rf"pub fn {name}\s*\(", rs), name
    assert re.search(r"pub fn sgx_fbank_create\([^)]*n_filters: u32,\s*h_first: \*const u32,\s*h_count: \*const u32,\s*h_weights: \*const f32,\s*"
                     r"power: u32,\s*out_fbank: \*mut \*mut SgxFbank\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_fbank_batch\(fbank: \*mut SgxFbank,[^)]*d_out: \*mut f32,\s*n_out: \*mut usize\)", rs)
    assert re.search(r"pub fn sgx_mel_weights\(sample_rate: f64,[^)]*n_weights: \*mut usize\)", rs)
    for name, value in (("SGX_MEL_HTK", 0), ("SGX_MEL_SLANEY", 1), ("SGX_MEL_NORM_NONE", 0), ("SGX_MEL_NORM_SLANEY", 1)):
        assert re.search(rf"pub const {name}: u32 = {value};", rs), name


def test_host_only_code_is_its_own_header():
    csrc = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "fbank_host.hpp"))
    assert "sgx_fbank.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        assert "sgx_fbank_batch" in text, doc
    assert "sgx_mel_weights" in _read("DESIGN.md") and "sgx_fbank_mags" in _read("DESIGN.md")
    assert "sgx_mel_weights" in _read("INTEGRATION.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "fbank_bench.py"))
