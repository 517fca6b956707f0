"""The root of unity the twiddle tables are made of -- csrc/unit_root.hpp -- as a stand-alone program (tests/cpp/unit_root_check.cpp, its
own main) built with g++ -fsanitize=address,undefined and run directly: every exponent of two turns at the table lengths the kernels
use.  Nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectrogram_rs_amd", "csrc")
LENGTHS = (256, 300, 512, 2048, 4096, 4800, 16384)


def test_every_point_is_the_rounded_double_angle_and_the_axes_are_exact(tmp_path):
    exe = str(tmp_path / "unit_root_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "unit_root_check.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "FAILED" not in p.stdout and "unit root ok" in p.stdout
    # every exponent in [0, 2n) of every length, eight of them on the axes (each length is a multiple of four)
    assert "%d points, %d on the axes, 0 failed" % (2 * sum(LENGTHS), 8 * len(LENGTHS)) in p.stdout
    assert all("%d," % n in open(os.path.join(ROOT, "tests", "cpp", "unit_root_check.cpp")).read().replace("};", ",") for n in LENGTHS)


def test_the_header_needs_no_hip_and_is_the_only_copy():
    """unit_root.hpp is what a plain C++ compiler reads; no translation unit keeps a lambda of its own"""
    text = open(os.path.join(CSRC, "unit_root.hpp")).read()
    assert "hip/" not in text and "__device__" not in text and "float2" not in text
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            assert "auto unit = [" not in open(os.path.join(CSRC, f)).read(), f
