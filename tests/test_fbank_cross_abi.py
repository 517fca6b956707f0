"""sgx_fbank_cross_* (per band the sums of |L|^2, |R|^2, Re and Im of L conj R, from PCM or from complex rows) through every layer,
without a GPU: the C header, the exports of libsgx.so, the ctypes table, FilterBank, the C++ mirror, the Rust binding and the
documents."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import FilterBank, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_fbank_cross_batch", "sgx_fbank_cross_spec", "sgx_fbank_cross_fused")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_cross_calls():
    h = _read("include", "sgx.h")
    assert re.search(r"SGX_API\s+int\s+sgx_fbank_cross_batch\s*\(\s*void\s*\*fbank,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*"
                     r"size_t first_frame,\s*size_t max_frames,\s*float\s*\*d_out,\s*size_t\s*\*n_out\)\s*;", h)
    assert re.search(r"SGX_API\s+int\s+sgx_fbank_cross_spec\s*\(\s*void\s*\*fbank,\s*const float\s*\*d_spec,\s*size_t n_columns,\s*float\s*\*d_out\)\s*;", h)
    assert re.search(r"SGX_API\s+int\s+sgx_fbank_cross_fused\s*\(\s*const void\s*\*fbank\)\s*;", h)
    # the conventions list names the two calls among those that only enqueue
    conventions = h.split("Conventions")[1].split("*/")[0]
    assert "sgx_fbank_cross_batch" in conventions and "sgx_fbank_cross_spec" in conventions
    # the definition lives in the filterbank section, between the magnitude bank's calls and the mel bank
    section = h[h.index("sgx_fbank_fused(const void *fbank);"):h.index("The triangular mel bank")]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for words in ("x0 = rn(rn(a * a) + rn(b * b))", "x1 = rn(rn(c * c) + rn(d * d))", "x2 = rn(rn(a * c) + rn(b * d))",
                  "x3 = rn(rn(b * c) - rn(a * d))", "no contraction into a fused multiply-add", "x0 = x1 = x2 and x3 = +0 exactly",
                  "bit for bit", "sgx_stft_batch_complex stores", "power plays no part", "four +0.0f", "pure function of the frame's complex row",
                  "[n_out][pairs][n_filters][4]", "[n_columns][M][2][2]", "[n_columns][n_filters][4]", "SGX_ERR_UNSUPPORTED",
                  "atan2(out3, out2)", "out2 / sqrt(out0 * out1)", "(out2 * out2 + out3 * out3) / (out0 * out1)",
                  "out0 + out1 + 2 * out2", "out0 + out1 - 2 * out2", "the caller's to guard", "nothing waits on the host",
                  "SGX_FLAG_NO_FUSED_RENDER", "SGX_FLAG_FORCE_GENERIC"):
        assert words in flat, words


def test_library_exports_the_cross_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig)
    assert all(sig[name][1] is ctypes.c_int for name in NEW)
    assert len(sig["sgx_fbank_cross_batch"][2]) == 7 and sig["sgx_fbank_cross_batch"][2][2] is ctypes.c_size_t
    assert sig["sgx_fbank_cross_batch"][2] == sig["sgx_fbank_batch"][2]
    assert len(sig["sgx_fbank_cross_spec"][2]) == 4 and sig["sgx_fbank_cross_spec"][2][2] is ctypes.c_size_t
    assert len(sig["sgx_fbank_cross_fused"][2]) == 1
    assert list(inspect.signature(FilterBank.cross_batch).parameters) == ["self", "pcm", "first_frame", "max_frames", "out"]
    batch = inspect.signature(FilterBank.cross_batch).parameters
    assert (batch["first_frame"].default, batch["max_frames"].default, batch["out"].default) == (0, None, None)
    assert list(inspect.signature(FilterBank.cross_apply).parameters) == ["self", "spec", "out"]
    assert isinstance(FilterBank.__dict__.get("cross_fused"), property)
    assert "sgx_fbank_cross_batch" in inspect.getsource(FilterBank.cross_batch)
    assert "sgx_fbank_cross_spec" in inspect.getsource(FilterBank.cross_apply)


def test_cpp_mirror_and_rust_binding():
    hpp = _read("include", "sgx.hpp")
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hpp), name
    bank = hpp[hpp.index("class FilterBank"):]
    for method in ("cross_batch", "cross_apply", "cross_fused"):
        assert re.search(rf"\b{method}\s*\(", bank), method
    rs = _read("bindings", "rust", "sgx_sys.rs")
    assert re.search(r"pub fn sgx_fbank_cross_batch\(fbank: \*mut SgxFbank,\s*d_pcm: \*const f32,\s*n_samples: usize,\s*first_frame: usize,\s*"
                     r"max_frames: usize,\s*d_out: \*mut f32,\s*n_out: \*mut usize\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_fbank_cross_spec\(fbank: \*mut SgxFbank,\s*d_spec: \*const f32,\s*n_columns: usize,\s*d_out: \*mut f32\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_fbank_cross_fused\(fbank: \*const SgxFbank\)\s*->\s*c_int", rs)


def test_device_code_is_where_the_design_says():
    csrc = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
    hpp, hip = _read(csrc, "sgx_fbank.hpp"), _read(csrc, "sgx_fbank.hip")
    assert "cross_filter_pass" in hpp and "fbank_cross_stage_kernel" in hip
    for intrinsic in ("__fmul_rn", "__fadd_rn", "__fsub_rn"):
        assert intrinsic in hpp, intrinsic
    assert "kPixFbankCross" in _read(csrc, "stft4096_wg.hpp") and "kPixFbankCross" in _read(csrc, "stft4096_wg.hip")
    assert "kFbankCross" in _read(csrc, "sgx_internal.hpp") and "Out::kFbankCross" in _read(csrc, "sgx_api.hip")


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        assert "sgx_fbank_cross_batch" in text, doc
    assert "sgx_fbank_cross_spec" in _read("DESIGN.md") and "sgx_fbank_cross_fused" in _read("DESIGN.md")
    assert "sgx_fbank_cross_spec" in _read("INTEGRATION.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "fbank_cross_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "fbank_cross.txt"))
