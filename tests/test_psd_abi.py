"""sgx_psd_* / sgx_csd_* (Welch-averaged spectra per bin: the mean over groups of frames of |X|^2 and of the four (L, R) products)
through every layer, without a GPU: the C header, the exports of libsgx.so, the ctypes table, the engine, the C++ mirror, the Rust
binding and the documents."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_psd_batch", "sgx_csd_batch", "sgx_psd_mags", "sgx_csd_spec", "sgx_psd_fused", "sgx_csd_fused")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_six_calls():
    h = _read("include", "sgx.h")
    for name, out in (("sgx_psd_batch", "d_psd"), ("sgx_csd_batch", "d_csd")):
        assert re.search(rf"SGX_API\s+int\s+{name}\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*size_t first_frame,\s*"
                         rf"size_t max_frames,\s*size_t group,\s*float\s*\*{out},\s*size_t\s*\*n_out\)\s*;", h), name
    assert re.search(r"SGX_API\s+int\s+sgx_psd_mags\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_mags,\s*size_t n_frames,\s*size_t group,\s*"
                     r"float\s*\*d_psd,\s*size_t\s*\*n_out\)\s*;", h)
    assert re.search(r"SGX_API\s+int\s+sgx_csd_spec\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_spec,\s*size_t n_frames,\s*size_t group,\s*"
                     r"float\s*\*d_csd,\s*size_t\s*\*n_out\)\s*;", h)
    for name in ("sgx_psd_fused", "sgx_csd_fused"):
        assert re.search(rf"SGX_API\s+int\s+{name}\s*\(\s*const sgx_ctx\s*\*ctx\)\s*;", h), name
    conventions = h.split("Conventions")[1].split("*/")[0]
    for name in NEW[:4]:
        assert name in conventions, name
    # the definition, its order included, and the scaling
    section = h[h.index("Welch-averaged spectra per bin"):h.index("SGX_API int sgx_psd_batch")]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for words in ("blocks of 32 consecutive frames counted from the column's first frame", "one chain of float32 adds from +0",
                  "s = rn(s + x)", "never contracted", "one chain of float64 adds from +0", "(float)(S / (double)n_j)",
                  "The block length 32 is fixed here", "compute-unit limit", "any split of a call at a column boundary", "bit for bit",
                  "x = rn(m * m)", "sgx_stft_batch stores", "sgx_stft_batch_complex stores", "group = 1 gives exactly rn(m * m)",
                  "35 * 2^-24", "group = 0: SGX_ERR_INVALID_ARG", "SIZE_MAX", "number of COLUMNS",
                  "(A * S1 / W)^2", "p * W^2 / (2 * S1^2)", "p * W^2 / (2 * fs * S2)", "No logarithm, no dB",
                  "[n_out][pairs][M][2]", "[n_out][pairs][M][4]", "16-byte aligned", "SGX_ERR_UNSUPPORTED", "(v, v)",
                  "[n_frames][pairs][M][2][2]", "nothing waits on the host", "192 MiB workspace", "one float64 row [pairs][M][4]",
                  "tests/test_gpu_psd.py", "tests/test_gpu_bounds.py", "test_gpu_stream_routes.py", "test_gpu_far_offsets.py",
                  "test_gpu_channel_counts.py", "test_gpu_cu_counts.py"):
        assert words in flat, words


def test_header_says_the_workspace_routes_take_the_rows_deal():
    h = _read("include", "sgx.h")
    flat = re.sub(r"\s*\n \*\s*", " ", h)
    claim = flat[flat.index("Diagnostic: how the rows calls"):flat.index("SGX_API int sgx_set_run_claim")]
    weights = flat[flat.index("Diagnostic: the weights of those calls"):flat.index("SGX_API int sgx_set_run_weights")]
    for words in ("The rows launches of the workspace routes take the same deal", "sgx_psd_batch always", "SGX_FLAG_NO_FUSED_RENDER",
                  "tests/test_gpu_claimed_runs.py", "holds those consumers to it"):
        assert words in claim, words
    for words in ("the rows launches of the workspace routes take the same deal", "the automatic one included", "tests/test_gpu_weighted_runs.py"):
        assert words in weights, words


def test_library_exports_the_six_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig)
    assert all(sig[name][1] is ctypes.c_int for name in NEW)
    assert sig["sgx_psd_batch"][2] == sig["sgx_csd_batch"][2] == sig["sgx_bands_peak_batch"][2]
    assert len(sig["sgx_psd_mags"][2]) == 6 and sig["sgx_psd_mags"][2] == sig["sgx_csd_spec"][2]
    assert sig["sgx_psd_mags"][2][2] is ctypes.c_size_t and sig["sgx_psd_mags"][2][3] is ctypes.c_size_t
    assert len(sig["sgx_psd_fused"][2]) == 1 and len(sig["sgx_csd_fused"][2]) == 1
    for method, call in (("psd_batch", "sgx_psd_batch"), ("csd_batch", "sgx_csd_batch")):
        fn = getattr(SpectrogramEngine, method)
        assert list(inspect.signature(fn).parameters) == ["self", "pcm", "group", "first_frame", "max_frames", "out"]
        p = inspect.signature(fn).parameters
        assert (p["first_frame"].default, p["max_frames"].default, p["out"].default) == (0, None, None)
        assert call in inspect.getsource(fn)
    assert list(inspect.signature(SpectrogramEngine.psd_mags).parameters) == ["self", "mags", "group", "out"]
    assert list(inspect.signature(SpectrogramEngine.csd_spec).parameters) == ["self", "spec", "group", "out"]
    assert "sgx_psd_mags" in inspect.getsource(SpectrogramEngine.psd_mags) and "sgx_csd_spec" in inspect.getsource(SpectrogramEngine.csd_spec)
    assert isinstance(SpectrogramEngine.__dict__.get("psd_fused"), property) and isinstance(SpectrogramEngine.__dict__.get("csd_fused"), property)


def test_cpp_mirror_and_rust_binding():
    hpp = _read("include", "sgx.hpp")
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hpp), name
    rs = _read("bindings", "rust", "sgx_sys.rs")
    for name, out in (("sgx_psd_batch", "d_psd"), ("sgx_csd_batch", "d_csd")):
        assert re.search(rf"pub fn {name}\(ctx: \*mut SgxCtx,\s*d_pcm: \*const f32,\s*n_samples: usize,\s*first_frame: usize,\s*max_frames: usize,\s*"
                         rf"group: usize,\s*{out}: \*mut f32,\s*n_out: \*mut usize\)\s*->\s*c_int", rs), name
    assert re.search(r"pub fn sgx_psd_mags\(ctx: \*mut SgxCtx,\s*d_mags: \*const f32,\s*n_frames: usize,\s*group: usize,\s*d_psd: \*mut f32,\s*"
                     r"n_out: \*mut usize\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_csd_spec\(ctx: \*mut SgxCtx,\s*d_spec: \*const f32,\s*n_frames: usize,\s*group: usize,\s*d_csd: \*mut f32,\s*"
                     r"n_out: \*mut usize\)\s*->\s*c_int", rs)
    for name in ("sgx_psd_fused", "sgx_csd_fused"):
        assert re.search(rf"pub fn {name}\(ctx: \*const SgxCtx\)\s*->\s*c_int", rs), name


def test_device_code_is_where_the_design_says():
    csrc = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
    hpp, hip = _read(csrc, "sgx_psd.hpp"), _read(csrc, "sgx_psd.hip")
    assert "block_chain" in hpp and "kBlock = 32" in hpp
    assert "__fadd_rn" in hpp and "__fmul_rn" in hpp and "cross_terms" in hpp
    assert "psd_block_kernel" in hip and "psd_combine_kernel" in hip and "__dadd_rn" in hip
    assert hip.count("block_chain(") == 1                                         # the only code that forms a block partial
    assert "sgx_psd.hip" in _read(csrc, "Makefile")
    assert "kPsd" in _read(csrc, "sgx_internal.hpp") and "kCsd" in _read(csrc, "sgx_internal.hpp")
    api = _read(csrc, "sgx_api.hip")
    assert "Out::kPsd" in api and "Out::kCsd" in api


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        assert "sgx_psd_batch" in text and "sgx_csd_batch" in text, doc
    for name in NEW:
        assert name in _read("DESIGN.md"), name
    assert "sgx_psd_mags" in _read("INTEGRATION.md") and "sgx_csd_spec" in _read("INTEGRATION.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "psd_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "psd.txt"))
