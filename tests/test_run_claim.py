"""The job split of a launch with a claimed tail -- csrc/run_claim.hpp, which the launcher and the kernel both read -- as a stand-alone program
(tests/cpp/run_claim_check.cpp, its own main) built with g++ -fsanitize=address,undefined and run directly: for n_jobs 0 .. 5000, workgroup
counts {1, 4, 1023, 1024}, static shares {0, 8, 12, 16} / 16 and chunks {1, 8, 64} every job is taken exactly once, no index leaves
[0, n_jobs), the static runs are contiguous, and the claim indices past the pool that every launch draws are empty runs.
Nothing is loaded into python and no HIP library is linked."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")


def test_every_job_is_taken_once_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "run_claim_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "run_claim_check.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "FAILED" not in p.stdout and "run claim ok" in p.stdout
    assert "%d splits checked" % (5001 * 4 * 4 * 3) in p.stdout


def test_the_header_is_plain_cpp():
    text = open(os.path.join(CSRC, "run_claim.hpp")).read()
    assert "#include" not in text and "__device__" not in text and "__global__" not in text and "hipError" not in text
