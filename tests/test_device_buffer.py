"""The one owner of device memory -- csrc/device_buffer.hpp -- as a stand-alone program (tests/cpp/device_buffer_check.cpp, its own main and
its own hipMalloc / hipFree / hipMemcpy / hipStreamSynchronize on malloc'd memory) built with g++ -fsanitize=address,undefined and run
directly: upload, moves, grow with an injected allocation failure, the two rules for an empty table, and no allocation alive at exit.
Nothing is loaded into python and no HIP library is linked."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")


def test_the_buffer_type_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "device_buffer_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "device_buffer_check.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "FAILED" not in p.stdout and "device buffer ok" in p.stdout
    for part in ("upload ok", "move ok", "grow ok", "empty ok", " 0 live"):
        assert part in p.stdout, part


def test_the_header_is_host_code_with_one_free():
    """device_buffer.hpp takes the runtime's declarations only, and frees in one place"""
    text = open(os.path.join(CSRC, "device_buffer.hpp")).read()
    assert "hip/hip_runtime.h" not in text and "__device__" not in text and "__global__" not in text
    assert text.count("hipFree(") == 1 and text.count("hipMalloc(") == 1
