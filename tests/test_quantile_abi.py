"""sgx_quantile_batch / sgx_quantile_mags / sgx_quantile_max_group (per-bin order statistics over groups of frames) through every layer,
without a GPU: the C header, the exports of libsgx.so, the ctypes table, the engine, the C++ mirror, the Rust binding, the documents, and
the refusals that need no device."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_quantile_batch", "sgx_quantile_mags", "sgx_quantile_max_group")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_three_calls():
    h = _read("include", "sgx.h")
    assert re.search(r"SGX_API\s+int\s+sgx_quantile_batch\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*size_t first_frame,\s*"
                     r"size_t max_frames,\s*size_t group,\s*const double\s*\*q,\s*uint32_t n_q,\s*float\s*\*d_out,\s*size_t\s*\*n_out\)\s*;", h)
    assert re.search(r"SGX_API\s+int\s+sgx_quantile_mags\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_mags,\s*size_t n_frames,\s*size_t group,\s*"
                     r"const double\s*\*q,\s*uint32_t n_q,\s*float\s*\*d_out,\s*size_t\s*\*n_out\)\s*;", h)
    assert re.search(r"SGX_API\s+size_t\s+sgx_quantile_max_group\s*\(\s*const sgx_ctx\s*\*ctx\)\s*;", h)
    conventions = h.split("Conventions")[1].split("*/")[0]
    for name in NEW[:2]:
        assert name in conventions, name
    # the definition: the wording is the contract
    section = h[h.index("Per-bin order statistics over groups of frames"):h.index("SGX_API int sgx_quantile_batch")]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for words in ("exactly as sgx_psd_batch", "the last column may be short", "group = 0 is SGX_ERR_INVALID_ARG", "*n_out is the number of columns",
                  "exactly the float32 words sgx_stft_batch stores",
                  "key(u) = u ^ (u >> 31 ? 0xffffffff : 0x80000000)", "compared as unsigned integers",
                  "-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN", "numeric order with NaN last, i.e. np.sort",
                  "n_q from 1 to 16", "in any order and may repeat", "k_i = (size_t)floor(q[i] * (double)(n_j - 1) + 0.5)",
                  "one double product, one add, one floor", "n_j = 2 and q = 0.5 gives k = 1", "q = 0 is the column's minimum and q = 1 its maximum",
                  "n_q = 0, n_q > 16, or any q that is NaN or outside [0, 1] is SGX_ERR_INVALID_ARG", "nothing is written or enqueued",
                  "The word of rank k_i in that order, bits unchanged", "no interpolation between ranks", "asks for both neighbours",
                  "route, launch geometry, compute-unit limit, run claim, run weights, stream, chunk seams and any split of a call at a column boundary",
                  "q is a host array, read before the call returns", "[n_out][n_q][pairs][M][2]", "no alignment beyond float's",
                  "sgx_render_mags, sgx_maxima_mags, sgx_fbank_mags and sgx_magnitude_in", "SGX_FLAG_PAIRED_FRAMES",
                  "Too few samples is *n_out = 0, not an error", "a null buffer or a null q is SGX_ERR_INVALID_ARG", "n_out may be NULL",
                  "192 MiB workspace", "A quantile does not decompose", "min(group, F) > sgx_quantile_max_group(ctx) is SGX_ERR_UNSUPPORTED",
                  "sgx_last_error names the cap", "at least 1", "[n_frames][pairs][M][2]", "Any group up to SIZE_MAX (one column)",
                  "every W the library accepts", "no workspace", "n_frames == 0: *n_out = 0 and SGX_OK", "nothing waits on the host",
                  "every kernel of a call goes onto the context's stream", "no fused mode and no flag",
                  "tests/test_gpu_quantile.py", "tests/quantile_reference.py"):
        assert words in flat, words


def test_library_exports_the_three_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name
    assert not hasattr(lib, "sgx_quantile_fused")                                 # no fused mode, no query for one


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig)
    assert sig["sgx_quantile_batch"][1] is ctypes.c_int and sig["sgx_quantile_mags"][1] is ctypes.c_int
    assert sig["sgx_quantile_max_group"][1] is ctypes.c_size_t and len(sig["sgx_quantile_max_group"][2]) == 1
    b, m, psd = sig["sgx_quantile_batch"][2], sig["sgx_quantile_mags"][2], sig["sgx_psd_batch"][2]
    assert len(b) == 10 and b[:6] == psd[:6] and b[8:] == psd[6:]
    assert b[6] is ctypes.POINTER(ctypes.c_double) and b[7] is ctypes.c_uint32
    assert len(m) == 8 and m[2] is ctypes.c_size_t and m[3] is ctypes.c_size_t and m[4] is ctypes.POINTER(ctypes.c_double) and m[5] is ctypes.c_uint32
    p = inspect.signature(SpectrogramEngine.quantile_batch).parameters
    assert list(p) == ["self", "pcm", "group", "q", "first_frame", "max_frames", "out"]
    assert (p["first_frame"].default, p["max_frames"].default, p["out"].default) == (0, None, None)
    p = inspect.signature(SpectrogramEngine.quantile_mags).parameters
    assert list(p) == ["self", "mags", "group", "q", "out"] and p["out"].default is None
    assert "sgx_quantile_batch" in inspect.getsource(SpectrogramEngine.quantile_batch)
    assert "sgx_quantile_mags" in inspect.getsource(SpectrogramEngine.quantile_mags)
    assert isinstance(SpectrogramEngine.quantile_max_group, property)


def test_refusals_that_need_no_device():
    lib = _lib.load()
    q = (ctypes.c_double * 1)(0.5)
    n_out = ctypes.c_size_t(7)
    assert lib.sgx_quantile_batch(None, None, 0, 0, 0, 1, q, 1, None, ctypes.byref(n_out)) == _lib.SGX_ERR_INVALID_ARG and n_out.value == 0
    n_out.value = 7
    assert lib.sgx_quantile_mags(None, None, 0, 1, q, 1, None, ctypes.byref(n_out)) == _lib.SGX_ERR_INVALID_ARG and n_out.value == 0
    assert lib.sgx_quantile_batch(None, None, 0, 0, 0, 1, q, 1, None, None) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_quantile_max_group(None) == 0


def test_cpp_mirror_and_rust_binding():
    hpp = _read("include", "sgx.hpp")
    for name in NEW + ("quantile_stream", "quantile_mags", "quantile_max_group"):
        assert re.search(rf"\b{name}\s*\(", hpp), name
    rs = _read("bindings", "rust", "sgx_sys.rs")
    assert re.search(r"pub fn sgx_quantile_batch\(ctx: \*mut SgxCtx,\s*d_pcm: \*const f32,\s*n_samples: usize,\s*first_frame: usize,\s*max_frames: usize,\s*"
                     r"group: usize,\s*q: \*const f64,\s*n_q: u32,\s*d_out: \*mut f32,\s*n_out: \*mut usize\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_quantile_mags\(ctx: \*mut SgxCtx,\s*d_mags: \*const f32,\s*n_frames: usize,\s*group: usize,\s*q: \*const f64,\s*n_q: u32,\s*"
                     r"d_out: \*mut f32,\s*n_out: \*mut usize\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_quantile_max_group\(ctx: \*const SgxCtx\)\s*->\s*usize", rs)


def test_device_code_is_where_the_design_says():
    csrc = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
    hpp, hip = _read(csrc, "sgx_quantile.hpp"), _read(csrc, "sgx_quantile.hip")
    assert "constexpr uint32_t kTile = 64" in hpp and "constexpr uint32_t kLdsFrames = 512" in hpp and "kMaxQ = 16" in hpp
    assert "select_keys" in hpp and "to_key" in hpp and "from_key" in hpp and "rank_of" in hpp
    assert hip.count("select_keys<") == 2, "one device function forms a result; both paths call it"
    assert "quantile_lds_kernel" in hip and "quantile_rows_kernel" in hip and "hipFuncSetAttribute" in hip and "lds_optin" in hip
    assert "sgx_quantile.hip" in _read(csrc, "Makefile")
    api = _read(csrc, "sgx_api.hip")
    body = api[api.index("int sgx_quantile_batch("):]
    body = body[:body.index("\n}\n")]
    assert "check_quantile(" in body and "begin_batch(" in body and "rows_to_workspace(" in body and "launch_quantile(" in body
    assert "SGX_ERR_UNSUPPORTED" in body and "quantile_cap(" in body
    stage = api[api.index("int sgx_quantile_mags("):]
    stage = stage[:stage.index("\n}\n")]
    assert "check_quantile(" in stage and "launch_quantile(" in stage and "workspace" not in stage
    # no new member of sgx::Out, no new flag, no query for a fused mode
    internal = _read(csrc, "sgx_internal.hpp")
    assert re.search(r"enum class Out \{ kMags, kMagsF16, kComplex, kRgba, kBands, kPeak, kFbank, kFbankCross, kPsd, kCsd \};", internal)
    assert "sgx_quantile_fused" not in _read("include", "sgx.h")


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        for name in NEW[:2]:
            assert name in text, (doc, name)
    design = _read("DESIGN.md")
    section = design[design.index("### Order statistics"):]
    section = section[:section.index("\n### ", 10)]
    for words in ("sgx_quantile.hip", "profiles/quantile.txt", "tools/quantile_bench.py", "tests/quantile_reference.py", "not measured",
                  "kLdsFrames", "kTile", "32 passes"):
        assert words in section, words
    assert "quantile_bench.py" in _read("tools", "README.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "quantile_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "quantile.txt"))
