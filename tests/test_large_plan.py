"""The plan rule of the multi-pass transform (spectrogram_rs_amd/csrc/large_plan.hpp, SGX_FLAG_LARGE_TRANSFORM), host code built with
g++ from the header where it lies: for every W in [4, 2^20] the factors are stage-engine lengths, their product is exactly 2W (or a
power of two >= 3W - 1 for chirp-z), and a workgroup's LDS image fits.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")


def test_plan_rule_for_every_window(tmp_path):
    exe = str(tmp_path / "large_plan_check")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "large_plan_check.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    assert p.stdout.startswith("plans ok"), p.stdout
    n_large = int(p.stdout.split()[2])
    assert n_large > 1_000_000    # nearly every W from 5462 to 2^20 needs the multi-pass transform
