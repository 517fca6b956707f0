"""The weighted deal of a rows launch -- csrc/run_claim.hpp: static runs sized by the workgroup's slot on its CU, which the launcher and the
kernel both read -- as a stand-alone program (tests/cpp/run_weights_check.cpp, its own main) built with g++ -fsanitize=address,undefined
and run directly: for n_jobs 0 .. 5000, (workgroups x CUs) {1x1, 4x1, 7x2, 8x2, 1023x256, 1024x256}, static shares {0, 8, 15, 16} / 16,
chunks {1, 8} and weights {(64,64,64,64), (88,80,48,40), (253,1,1,1), (1,1,1,253)} every job is taken exactly once, no index leaves
[0, n_jobs), the static runs are contiguous and in block order, share 16 partitions exactly with an empty pool, and equal weights with a
pool give exactly static_run / claimed_run of run_claim.  Nothing is loaded into python and no HIP library is linked."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")


def test_every_weighted_deal_takes_every_job_once_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "run_weights_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "run_weights_check.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "FAILED" not in p.stdout and "run weights ok" in p.stdout
    assert "%d deals checked" % (5001 * 6 * 4 * 2 * 4) in p.stdout


def test_the_header_is_still_plain_cpp():
    text = open(os.path.join(CSRC, "run_claim.hpp")).read()
    assert "#include" not in text and "__device__" not in text and "__host__" not in text and "__global__" not in text and "hipError" not in text
    assert "blockIdx" not in text and "threadIdx" not in text and "hipLaunch" not in text
