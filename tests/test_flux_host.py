"""The host-only half of sgx_flux_batch -- how a call is cut into ranges whose rows, predecessors included, fit the workspace, and
sgx_flux_max_lag: csrc/flux_host.hpp -- as a stand-alone program (tests/cpp/flux_host_check.cpp, its own main) built with
g++ -fsanitize=address,undefined and run directly.  Nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")


def test_the_range_arithmetic_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "flux_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "flux_host_check.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "flux host ok" in p.stdout and "FAILED" not in p.stdout
    for line in ("max_lag ok", "small calls ok", "context caps ok", "far frames ok"):
        assert line in p.stdout, line


def test_the_header_needs_no_hip():
    """flux_host.hpp is what a plain C++ compiler reads: no HIP header, no device attribute"""
    text = open(os.path.join(CSRC, "flux_host.hpp")).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
    # and the dispatch holds its own workspace size to the header's
    api = open(os.path.join(CSRC, "sgx_api.hip")).read()
    assert "flux::range_at" in api and "flux::max_lag" in api and "flux::kWorkspaceBytes == kWorkspaceBytes" in api
