"""sgx_flux_* (per band the rise and the fall of every bin against the same bin `lag` frames earlier, from PCM or from magnitude
rows) through every layer, without a GPU: the C header, the exports of libsgx.so, the null-handle answers, the ctypes table, FilterBank,
the C++ mirror, the Rust binding, where the device code lives, and the documents."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import FilterBank, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_flux_batch", "sgx_flux_mags", "sgx_flux_max_lag")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_flux_calls():
    h = _read("include", "sgx.h")
    assert re.search(r"SGX_API\s+int\s+sgx_flux_batch\s*\(\s*void\s*\*fbank,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*size_t first_frame,\s*"
                     r"size_t max_frames,\s*uint32_t lag,\s*float\s*\*d_out,\s*size_t\s*\*n_out\)\s*;", h)
    assert re.search(r"SGX_API\s+int\s+sgx_flux_mags\s*\(\s*void\s*\*fbank,\s*const float\s*\*d_mags,\s*size_t n_frames,\s*uint32_t lag,\s*"
                     r"float\s*\*d_out\)\s*;", h)
    assert re.search(r"SGX_API\s+uint32_t\s+sgx_flux_max_lag\s*\(\s*const void\s*\*fbank\)\s*;", h)
    # the conventions list names the two calls among those that only enqueue
    conventions = h.split("Conventions")[1].split("*/")[0]
    assert "sgx_flux_batch" in conventions and "sgx_flux_mags" in conventions
    # the definition lives in the filterbank section, between the cross sums and the mel bank
    section = h[h.index("sgx_fbank_cross_fused(const void *fbank);"):h.index("The triangular mel bank")]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for words in ("x_t[j]  = m (power 1) or rn(m * m) (power 2)", "d[j]    = rn(x_t[j] - x_{t - lag}[j])", "never contracted",
                  "rise[j] = d < 0 ? +0 : d", "fall[j] = d > 0 ? +0 : rn(+0 - d)", "never -0", "NaN in either row gives NaN in both",
                  "(rise_l, rise_r, fall_l, fall_r)", "the 64 chains from +0, then the tree by halving", "count == 0 gives four +0.0f",
                  "t < lag has no predecessor", "(+0, +0, +0, +0)", "pure function of the two rows and the bank", "bit for bit",
                  "rise - fall telescopes", "weighted L1 distance", "full-band spectral flux", "no logarithm", "no normalisation", "no peak picking",
                  "payload of a resulting NaN is unspecified", "no fused mode, no flag and no query",
                  "[n_out][pairs][n_filters][4]", "16-byte aligned", "[n_frames][pairs][M][2]", "[n_frames][pairs][n_filters][4]",
                  "rise_l = rise_r", "SGX_FLAG_PAIRED_FRAMES", "lag == 0 or lag > 64 is SGX_ERR_INVALID_ARG",
                  "reads frame first_frame - lag out of the PCM itself", "any split of a call concatenates to the whole call",
                  "min(64, floor(192 MiB / bytes of one frame's rows) - 1)", "23 at W = 2^20 with two channels", "SGX_ERR_UNSUPPORTED",
                  "recomputed, not carried", "nothing waits on the host", "n_frames == 0 is SGX_OK"):
        assert words in flat, words


def test_library_exports_the_flux_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name
    assert not hasattr(lib, "sgx_flux_fused"), "the flux has no fused mode and no query for one"


def test_null_handle_calls():
    """answered before any device is looked at"""
    lib = _lib.load()
    got = ctypes.c_size_t(7)
    dummy = (ctypes.c_float * 8)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    assert lib.sgx_flux_batch(None, p, 4096, 0, 1, 1, p, ctypes.byref(got)) == _lib.SGX_ERR_INVALID_ARG and got.value == 0
    assert lib.sgx_flux_batch(None, p, 4096, 0, 1, 1, p, None) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_flux_mags(None, p, 1, 1, p) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_flux_max_lag(None) == 0
    assert not any(dummy)


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig)
    assert sig["sgx_flux_batch"][1] is ctypes.c_int and sig["sgx_flux_mags"][1] is ctypes.c_int
    assert sig["sgx_flux_max_lag"][1] is ctypes.c_uint32 and len(sig["sgx_flux_max_lag"][2]) == 1
    batch = sig["sgx_flux_batch"][2]
    assert len(batch) == 8 and batch[2] is ctypes.c_size_t and batch[5] is ctypes.c_uint32
    assert batch[:5] == sig["sgx_fbank_batch"][2][:5] and batch[6:] == sig["sgx_fbank_batch"][2][5:]      # sgx_fbank_batch's with the lag put in
    mags = sig["sgx_flux_mags"][2]
    assert len(mags) == 5 and mags[2] is ctypes.c_size_t and mags[3] is ctypes.c_uint32
    assert list(inspect.signature(FilterBank.flux_batch).parameters) == ["self", "pcm", "lag", "first_frame", "max_frames", "out"]
    batch = inspect.signature(FilterBank.flux_batch).parameters
    assert (batch["lag"].default, batch["first_frame"].default, batch["max_frames"].default, batch["out"].default) == (1, 0, None, None)
    assert list(inspect.signature(FilterBank.flux_apply).parameters) == ["self", "mags", "lag", "out"]
    apply = inspect.signature(FilterBank.flux_apply).parameters
    assert (apply["lag"].default, apply["out"].default) == (1, None)
    assert isinstance(FilterBank.__dict__.get("flux_max_lag"), property)
    assert "flux_fused" not in FilterBank.__dict__
    assert "sgx_flux_batch" in inspect.getsource(FilterBank.flux_batch)
    assert "sgx_flux_mags" in inspect.getsource(FilterBank.flux_apply)


def test_cpp_mirror_and_rust_binding():
    hpp = _read("include", "sgx.hpp")
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hpp), name
    bank = hpp[hpp.index("class FilterBank"):]
    for method in ("flux_batch", "flux_apply", "flux_max_lag"):
        assert re.search(rf"\b{method}\s*\(", bank), method
    rs = _read("bindings", "rust", "sgx_sys.rs")
    assert re.search(r"pub fn sgx_flux_batch\(fbank: \*mut SgxFbank,\s*d_pcm: \*const f32,\s*n_samples: usize,\s*first_frame: usize,\s*"
                     r"max_frames: usize,\s*lag: u32,\s*d_out: \*mut f32,\s*n_out: \*mut usize\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_flux_mags\(fbank: \*mut SgxFbank,\s*d_mags: \*const f32,\s*n_frames: usize,\s*lag: u32,\s*d_out: \*mut f32\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_flux_max_lag\(fbank: \*const SgxFbank\)\s*->\s*u32", rs)


def test_device_code_is_where_the_design_says():
    csrc = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
    hpp, hip, api = _read(csrc, "sgx_fbank.hpp"), _read(csrc, "sgx_fbank.hip"), _read(csrc, "sgx_api.hip")
    assert "struct FluxRows" in hpp and "flux_terms" in hpp and "__fsub_rn" in hpp[hpp.index("flux_element"):]
    assert "fbank_flux_stage_kernel" in hip and "launch_fbank_flux_stage" in hip and "launch_fbank_flux_stage" in hpp
    kernel = hip[hip.index("fbank_flux_stage_kernel"):hip.index("hipError_t launch_fbank_flux_stage")]
    assert "cross_filter_pass(fbank::CrossColumns{rise, fall}" in kernel and "cross_filter_pass(fbank::FluxRows{" in kernel
    # one launch function for the batch route and the stage call: it takes the head rows to skip
    assert api.count("launch_fbank_flux_stage(") == 2 and "r.back, r.m, lag" in api
    assert "rows_to_workspace(c, d_pcm, r.a - r.back, r.back + r.m, total)" in api
    # the output kinds keep their ten members: the flux is a stage of a bank, not a route of the transforms
    internal = _read(csrc, "sgx_internal.hpp")
    assert "Flux" not in internal[internal.index("enum class Out"):].split("};")[0]
    assert os.path.exists(os.path.join(csrc, "flux_host.hpp"))


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        assert "sgx_flux_batch" in text, doc
    design = _read("DESIGN.md")
    assert "### Flux of a bank" in design and "sgx_flux_mags" in design and "sgx_flux_max_lag" in design
    assert "recomputed" in design[design.index("### Flux of a bank"):]
    assert "sgx_flux_mags" in _read("INTEGRATION.md")
    assert "flux_bench.py" in _read("tools", "README.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "flux_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "flux.txt"))
