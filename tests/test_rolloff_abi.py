"""sgx_rolloff_batch / sgx_rolloff_mags (where a frame's cumulative spectrum crosses shares of its total) through every layer, without a
GPU: the C header, the exports of libsgx.so, the ctypes table, the engine, the C++ mirror, the Rust binding and the documents."""
import ctypes
import inspect
import os
import re

from spectrogram_rs_amd import SpectrogramEngine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgx_rolloff_batch", "sgx_rolloff_mags")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_two_calls():
    h = _read("include", "sgx.h")
    assert re.search(r"SGX_API\s+int\s+sgx_rolloff_batch\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_pcm,\s*size_t n_samples,\s*size_t first_frame,\s*"
                     r"size_t max_frames,\s*uint32_t power,\s*const float\s*\*h_p,\s*uint32_t n_p,\s*float\s*\*d_out,\s*size_t\s*\*n_out\)\s*;", h)
    assert re.search(r"SGX_API\s+int\s+sgx_rolloff_mags\s*\(\s*sgx_ctx\s*\*ctx,\s*const float\s*\*d_mags,\s*size_t n_columns,\s*uint32_t power,\s*"
                     r"const float\s*\*h_p,\s*uint32_t n_p,\s*float\s*\*d_out\)\s*;", h)
    conventions = h.split("Conventions")[1].split("*/")[0]
    for name in NEW:
        assert name in conventions, name
    # the definition, its order included
    section = h[h.index("The cumulative spectrum per frame"):h.index("SGX_API int sgx_rolloff_batch")]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for words in ("exactly the float32 words that sgx_stft_batch stores", "bin k = j + 1", "The order below is part of the definition",
                  "x[j] = m[j] (power 1) or rn(m[j] * m[j]) (power 2", "never contracted into the add", "Any other power is SGX_ERR_INVALID_ARG",
                  "segments of S = 32 consecutive elements counted from element 0", "the last may be short",
                  "s[b][i] = rn(s[b][i-1] + x[32 b + i])", "o[0] = +0 and o[b+1] = rn(o[b] + s[b][last i of b])",
                  "c[j] = rn(o[b] + s[b][i]) for j = 32 b + i", "T = c[M-1], not a separately formed sum", "c never decreases",
                  "rn is monotone", "so it EQUALS o[b+1]", "S = 32 is fixed here",
                  "does not depend on the device, the route, the launch geometry or M", "np.cumsum", "tests/rolloff_reference.py",
                  "n_p from 1 to 8", "float32 in (0, 1]", "in any order and possibly repeated", "thr = rn(p[i] * T): one float32 product",
                  "n_p = 0, n_p > 8, or any p that is NaN or outside (0, 1] is SGX_ERR_INVALID_ARG", "nothing is written or enqueued",
                  "h_p is a host array, read before the call returns", "the smallest j with c[j] >= thr",
                  "((float)(j* + 1), c[j* - 1], c[j*], T)", "+0 in place of c[-1]", "the record is (0, 0, 0, T)",
                  "k = 0 is never a stored bin", "Every record is always written", "are unspecified", "infinities follow IEEE arithmetic",
                  "pure function of the row, bit for bit", "no interpolation and no conversion to Hz",
                  "[n_out][pairs][2][n_p][4]", "16-byte aligned", "nothing written", "same records on both sides", "SGX_FLAG_PAIRED_FRAMES",
                  "too few samples is *n_out = 0, not an error", "a null h_p is SGX_ERR_INVALID_ARG", "[n_columns][pairs][M][2]",
                  "SGX_FLAG_LARGE_TRANSFORM lengths included", "n_columns == 0: SGX_OK", "nothing waits on the host",
                  "every kernel of a call goes onto the context's stream", "192 MiB workspace only",
                  "no fused mode, no flag and no query for one", "tests/test_gpu_rolloff.py"):
        assert words in flat, words


def test_library_exports_the_two_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "spectrogram_rs_amd", "libsgx.so"))
    for name in NEW:
        assert hasattr(lib, name), name
    assert not hasattr(lib, "sgx_rolloff_fused")                                  # no fused mode, no query for one
    assert "sgx_rolloff_fused" not in _read("include", "sgx.h")


def test_python_bindings():
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert set(NEW) <= set(sig) and "sgx_rolloff_fused" not in sig
    assert all(sig[name][1] is ctypes.c_int for name in NEW)
    b, m = sig["sgx_rolloff_batch"][2], sig["sgx_rolloff_mags"][2]
    fp = ctypes.POINTER(ctypes.c_float)
    assert len(b) == 10 and b[:5] == sig["sgx_stft_batch"][2][:5]
    assert b[5] is ctypes.c_uint32 and b[6] is fp and b[7] is ctypes.c_uint32 and b[8:] == sig["sgx_stft_batch"][2][5:]
    assert len(m) == 7 and m[:2] == b[:2] and m[2] is ctypes.c_size_t and m[3] is ctypes.c_uint32 and m[4] is fp and m[5] is ctypes.c_uint32
    assert m[6] is b[8]
    p = inspect.signature(SpectrogramEngine.rolloff_batch).parameters
    assert list(p) == ["self", "pcm", "power", "p", "first_frame", "max_frames", "out"]
    assert (p["first_frame"].default, p["max_frames"].default, p["out"].default) == (0, None, None)
    p = inspect.signature(SpectrogramEngine.rolloff_mags).parameters
    assert list(p) == ["self", "mags", "power", "p", "out"] and p["out"].default is None
    assert "sgx_rolloff_batch" in inspect.getsource(SpectrogramEngine.rolloff_batch)
    assert "sgx_rolloff_mags" in inspect.getsource(SpectrogramEngine.rolloff_mags)
    assert not hasattr(SpectrogramEngine, "rolloff_fused")


def test_cpp_mirror_and_rust_binding():
    hpp = _read("include", "sgx.hpp")
    for name in NEW + ("rolloff_stream", "rolloff_mags"):
        assert re.search(rf"\b{name}\s*\(", hpp), name
    rs = _read("bindings", "rust", "sgx_sys.rs")
    assert re.search(r"pub fn sgx_rolloff_batch\(ctx: \*mut SgxCtx,\s*d_pcm: \*const f32,\s*n_samples: usize,\s*first_frame: usize,\s*max_frames: usize,\s*"
                     r"power: u32,\s*h_p: \*const f32,\s*n_p: u32,\s*d_out: \*mut f32,\s*n_out: \*mut usize\)\s*->\s*c_int", rs)
    assert re.search(r"pub fn sgx_rolloff_mags\(ctx: \*mut SgxCtx,\s*d_mags: \*const f32,\s*n_columns: usize,\s*power: u32,\s*h_p: \*const f32,\s*"
                     r"n_p: u32,\s*d_out: \*mut f32\)\s*->\s*c_int", rs)


def test_device_code_is_where_the_design_says():
    csrc = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
    hpp, hip = _read(csrc, "sgx_rolloff.hpp"), _read(csrc, "sgx_rolloff.hip")
    assert "kSegment = 32" in hpp and "kMaxShares = 8" in hpp
    assert "rolloff_kernel" in hip and "__fadd_rn" in hip and "__fmul_rn" in hip and "__ballot" in hip and "float4" in hip and "float2" in hip
    assert "asm" not in hip
    assert "sgx_rolloff.hip" in _read(csrc, "Makefile")
    api = _read(csrc, "sgx_api.hip")
    body = api[api.index("int sgx_rolloff_batch("):]
    body = body[:body.index("\n}\n")]
    assert "begin_batch(" in body and "in_workspace_chunks(" in body and "rows_to_workspace(" in body and "launch_rolloff(" in body
    # no new member of sgx::Out, no new flag
    internal = _read(csrc, "sgx_internal.hpp")
    assert re.search(r"enum class Out \{ kMags, kMagsF16, kComplex, kRgba, kBands, kPeak, kFbank, kFbankCross, kPsd, kCsd \};", internal)


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        for name in NEW:
            assert name in text, (doc, name)
    design = _read("DESIGN.md")
    section = design[design.index("### Cumulative spectrum"):]
    section = section[:section.index("\n### ", 10)] if "\n### " in section[10:] else section
    for words in ("sgx_rolloff.hip", "profiles/rolloff.txt", "tools/rolloff_bench.py", "tests/rolloff_reference.py", "not measured"):
        assert words in section, words
    assert "rolloff_bench.py" in _read("tools", "README.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "rolloff_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "rolloff.txt"))
