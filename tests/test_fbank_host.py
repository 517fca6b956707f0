"""The host-only half of the filterbank calls -- bank validation and sgx_mel_weights, csrc/fbank_host.hpp -- as a stand-alone program
(tests/cpp/fbank_host_check.cpp, its own main) built with g++ -fsanitize=address,undefined and run directly: the mel cases of
tests/test_fbank_mel.py on exactly sized heap arrays, every invalid argument, and the validation of a bank.  Nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")


def test_validation_and_mel_weights_are_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fbank_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "fbank_host_check.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "fbank host ok" in p.stdout and "FAILED" not in p.stdout
    assert p.stdout.count("mel ok") == 5 * 2 * 2 and "mel invalid ok" in p.stdout and "validation ok" in p.stdout
    assert p.stdout.count(", 6 empty") == 2 and p.stdout.count(", 7 empty") == 2     # W 64, 40 mels: filters narrower than the bin spacing


def test_the_header_needs_no_hip():
    """fbank_host.hpp is what a plain C++ compiler reads: no HIP header, no device attribute"""
    text = open(os.path.join(CSRC, "fbank_host.hpp")).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
