"""sgx_maxima_batch / sgx_maxima_mags (the K strongest spectral maxima per frame, pair and side) through every layer, without a GPU: the C
header, the exports of libsgx.so, the ctypes table, the engine, the C++ mirror, the Rust binding and the documents."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_maxima_batch", "sgx_maxima_mags")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_two_calls():
    h = _read("include", "sgx.h")
    assert re.search(r"SGX_API\s+int\s+sgx_maxima_batch\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*size_t first_frame,\s*"
                     r"size_t max_frames,\s*uint32_t k,\s*float floor,\s*float\s*\*d_max,\s*size_t\s*\*n_out\)\s*;", h)
    assert re.search(r"SGX_API\s+int\s+sgx_maxima_mags\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_mags,\s*size_t n_columns,\s*uint32_t k,\s*"
                     r"float floor,\s*float\s*\*d_max\)\s*;", h)
    conventions = h.split("Conventions")[1].split("*/")[0]
    for name in NEW:
        assert name in conventions, name
    # the definition, its order included
    section = h[h.index("The K strongest spectral maxima per frame"):h.index("SGX_API int sgx_maxima_batch")]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for words in ("exactly the float32 values that sgx_stft_batch stores", "bin k = j + 1", "The order below is part of the definition",
                  "An interior j (1 <= j <= M - 2) is a candidate when all three hold", "m[j] > m[j-1], m[j] >= m[j+1] and m[j] >= floor",
                  "A plateau yields its leftmost bin only", "Bins 1 and W - 1 are never candidates", "Where M < 3 there are none",
                  "descending m[j], ties by ascending j", "the first K are the result", "pure function of the row, bit for bit",
                  "route, launch geometry, compute-unit limit, run claim, run weights, stream, chunk seams and any split of a call",
                  "((float)k, m[j-1], m[j], m[j+1])", "no interpolation, logarithm or division", "is the caller's, from the three values",
                  "hold (0, 0, 0, 0)", "k = 0 is never a stored bin", "All K slots are always written",
                  "K from 1 to 64", "K = 0 or K > 64 is SGX_ERR_INVALID_ARG", "floor is finite and >= 0, else SGX_ERR_INVALID_ARG",
                  "is unspecified", "[n_out][pairs][2][K][4]", "16-byte aligned", "nothing written", "same records on both sides",
                  "SGX_FLAG_PAIRED_FRAMES", "too few samples is *n_out = 0, not an error", "[n_columns][pairs][M][2]",
                  "SGX_FLAG_LARGE_TRANSFORM lengths included", "n_columns == 0: SGX_OK", "nothing waits on the host",
                  "every kernel of a call goes onto the context's stream", "192 MiB workspace only", "no fused mode and no flag",
                  "tests/test_gpu_maxima.py", "tests/maxima_reference.py"):
        assert words in flat, words


def test_library_exports_the_two_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name
    assert not hasattr(lib, "sgx_maxima_fused")                                   # no fused mode, no query for one


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig)
    assert all(sig[name][1] is ctypes.c_int for name in NEW)
    b, m = sig["sgx_maxima_batch"][2], sig["sgx_maxima_mags"][2]
    assert len(b) == 9 and b[:5] == sig["sgx_stft_batch"][2][:5]
    assert b[5] is ctypes.c_uint32 and b[6] is ctypes.c_float and b[7:] == sig["sgx_stft_batch"][2][5:]
    assert len(m) == 6 and m[2] is ctypes.c_size_t and m[3] is ctypes.c_uint32 and m[4] is ctypes.c_float
    p = inspect.signature(SpectrogramEngine.maxima_batch).parameters
    assert list(p) == ["self", "pcm", "k", "floor", "first_frame", "max_frames", "out"]
    assert (p["floor"].default, p["first_frame"].default, p["max_frames"].default, p["out"].default) == (0.0, 0, None, None)
    p = inspect.signature(SpectrogramEngine.maxima_mags).parameters
    assert list(p) == ["self", "mags", "k", "floor", "out"] and (p["floor"].default, p["out"].default) == (0.0, None)
    assert "sgx_maxima_batch" in inspect.getsource(SpectrogramEngine.maxima_batch)
    assert "sgx_maxima_mags" in inspect.getsource(SpectrogramEngine.maxima_mags)


def test_cpp_mirror_and_rust_binding():
    hpp = _read("include", "sgx.hpp")
    for name in NEW + ("maxima_stream", "maxima_mags"):
        assert re.search(rf"\b{name}\s*\(", hpp), name
    rs = _read("bindings", "rust", "sgx_sys.rs")
    assert re.search(r"pub fn sgx_maxima_batch\(ctx: \*mut SgxCtx,\s*d_pcm: \*const f32,\s*n_samples: usize,\s*first_frame: usize,\s*max_frames: usize,\s*"
                     r"k: u32,\s*floor: f32,\s*d_max: \*mut f32,\s*n_out: \*mut usize\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_maxima_mags\(ctx: \*mut SgxCtx,\s*d_mags: \*const f32,\s*n_columns: usize,\s*k: u32,\s*floor: f32,\s*"
                     r"d_max: \*mut f32\)\s*->\s*c_int", rs)


def test_device_code_is_where_the_design_says():
    csrc = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
    hpp, hip = _read(csrc, "sgx_maxima.hpp"), _read(csrc, "sgx_maxima.hip")
    assert "make_key" in hpp and "0xffffffffu - j" in hpp and "kMaxK = 64" in hpp
    assert "maxima_kernel" in hip and "wave_max" in hip and "float4" in hip and "float2" in hip
    assert "sgx_maxima.hip" in _read(csrc, "Makefile")
    api = _read(csrc, "sgx_api.hip")
    body = api[api.index("int sgx_maxima_batch("):]
    body = body[:body.index("\n}\n")]
    assert "begin_batch(" in body and "in_workspace_chunks(" in body and "rows_to_workspace(" in body and "launch_maxima(" in body
    # no new member of sgx::Out, no new flag, no query for a fused mode
    internal = _read(csrc, "sgx_internal.hpp")
    assert re.search(r"enum class Out \{ kMags, kMagsF16, kComplex, kRgba, kBands, kPeak, kFbank, kFbankCross, kPsd, kCsd \};", internal)
    assert "sgx_maxima_fused" not in _read("include", "sgx.h")


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        for name in NEW:
            assert name in text, (doc, name)
    design = _read("DESIGN.md")
    section = design[design.index("### Spectral maxima"):]
    section = section[:section.index("\n### ", 10)]
    for words in ("sgx_maxima.hip", "profiles/maxima.txt", "tools/maxima_bench.py", "tests/maxima_reference.py", "not measured"):
        assert words in section, words
    assert "maxima_bench.py" in _read("tools", "README.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "maxima_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "maxima.txt"))
