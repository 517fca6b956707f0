"""The edge streams of tests/edge_signals.py have teeth (no GPU): on every row of the route table each target offset is covered, every
simulated misread of a target sample moves the float64 truth by >= 100 x the row's allowance, and the sentinels on the window's exact
zeros change nothing -- unless the window there is not exactly zero.  tests/test_gpu_edges.py then holds every route to these streams."""
import os
import subprocess

import numpy as np
import pytest

import edge_signals as es
import oracle
from conftest import mags_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEETH = 100.0          # the least error, in allowances, that a simulated misread must produce
BIG_W = 65537          # above this, the sensitivity checks take a handful of offsets (a 2^21-point FFT per misread)


def _stream(name):
    return _streams.setdefault(name, es.build_stream(es.ROUTE[name]))


_streams = {}
ROWS = [r.name for r in es.ROUTES]


def _window_nonzeros(s, t):
    """(offset, channel) of every sample of frame t whose windowed value is non-zero"""
    x = s.frame(t)
    return [tuple(int(v) for v in ij) for ij in np.argwhere(x * es.hann(s.route.W)[:, None] != 0)]


@pytest.mark.parametrize("name", ROWS)
def test_coverage(name):
    s = _stream(name)
    r = s.route
    W, H = r.W, r.H
    assert s.pcm.shape == ((s.frames - 1) * H + W, r.channels)             # ends with the last frame's last sample
    assert np.isfinite(s.pcm).all()
    targets = s.target_slots()
    frames_of = {}
    for sl in targets:
        nz = _window_nonzeros(s, sl.frame)
        # exactly two non-zero samples in the whole window, the pair, on one channel, each windowed to about +-1
        assert sorted(nz) == sorted([(sl.n, sl.channel), (sl.m, sl.channel)]), (name, sl)
        for off in (sl.n, sl.m):
            v = np.float64(s.pcm[sl.frame * H + off, sl.channel] * es.hann(W)[off])
            assert abs(abs(v) - 1.0) < 1e-6, (name, sl, off, v)
        frames_of.setdefault(sl.n, []).append(sl.frame)
    for n in s.E:
        assert n in frames_of, (name, n)
        if r.paired:   # in the even and in the odd frame of a transform
            assert {t % 2 for t in frames_of[n]} == {0, 1}, (name, n, frames_of[n])
    assert {sl.frame for sl in targets} >= {0, s.frames - 1}
    # sentinels: every offset of Z, every channel, in some frame; finite
    sent = [sl for sl in s.slots if sl.kind == "sentinel"]
    assert sent and s.Z and s.Z[0] == 0
    for z in s.Z:
        for c in range(r.channels):
            assert any(s.pcm[sl.frame * H + z, c] != 0 for sl in sent), (name, z, c)
    # frames with no non-zero windowed sample at all
    silent = [t for t in range(s.frames) if es.windowed_silent(s.frame(t), W).all()]
    assert len(silent) >= 1, name
    # pairs cycle through every channel
    assert {sl.channel for sl in targets} == set(range(r.channels)), name
    if r.chunk_targets:
        assert s.frames >= r.min_frames
        bounds = es.chunk_boundary_frames(W, r.pairs, s.frames)
        assert bounds and set(bounds) <= {sl.frame for sl in targets}, (name, bounds)


def _sensitivity_slots(s):
    firsts = {}
    for sl in s.target_slots():
        firsts.setdefault(sl.n, sl)
    if s.route.W <= BIG_W:
        return list(firsts.values())
    E = s.E
    pick = E[:2] + E[es.N_TARGET_EDGE:es.N_TARGET_EDGE + 2] + [s.route.W // 2] + E[2 * es.N_TARGET_EDGE + 1:2 * es.N_TARGET_EDGE + 3]
    return [firsts[n] for n in pick]


def _misreads(x, n, ch, W):
    """simulated misreads of the sample at (n, ch): dropped, moved by one position, moved to the other channel of its pair"""
    out = {}
    y = x.copy()
    y[n, ch] = 0
    out["zeroed"] = y
    for d in (-1, 1):
        if 0 <= n + d < W:
            y = x.copy()
            y[n + d, ch], y[n, ch] = x[n, ch], 0
            out["moved %+d" % d] = y
    if x.shape[1] > 1:
        y = x.copy()
        y[n, ch ^ 1], y[n, ch] = x[n, ch], 0
        out["other channel"] = y
    return out


@pytest.mark.parametrize("name", ROWS)
def test_sensitivity(name):
    s = _stream(name)
    r = s.route
    worst = np.inf
    for sl in _sensitivity_slots(s):
        x = s.frame(sl.frame)
        pair = sl.channel // 2
        clean = es.truth_frame(es.frame_lr(x, pair), r.W)
        for what, y in _misreads(x, sl.n, sl.channel, r.W).items():
            err = mags_error(es.truth_frame(es.frame_lr(y, pair), r.W), clean, r.floor)
            assert err >= TEETH, (name, sl.n, what, err)
            worst = min(worst, err)
    print(f"{name}: least misread error {worst:.3g} x")


@pytest.mark.parametrize("name", ROWS)
def test_sentinels(name):
    s = _stream(name)
    r = s.route
    Z = list(s.Z)
    for sl in (x for x in s.slots if x.kind == "sentinel"):
        x = s.frame(sl.frame)
        for pair in range(r.pairs):
            clean = es.truth_frame(es.frame_lr(x, pair), r.W)
            for other in (0.0, -3.0e37, 12345.0):
                y = x.copy()
                y[Z, :] = np.float32(other)
                assert np.array_equal(es.truth_frame(es.frame_lr(y, pair), r.W), clean), (name, other)
            win = es.hann(r.W).copy()
            win[Z] = np.float32(1e-8)      # a window that is tiny, not zero, on Z
            err = mags_error(es.truth_frame(es.frame_lr(x, pair), r.W, win), clean, r.floor)
            assert err >= TEETH, (name, pair, err)


@pytest.mark.parametrize("name", ["k1r_h256", "k16_ch8_h300", "bluestein_w23", "large_w65537_chirp_lr"])
def test_truth_is_the_oracles(name):
    # the windowed truth of these tests is oracle.np_truth_frame, bit for bit
    s = _stream(name)
    for sl in s.slots[:3] + [x for x in s.slots if x.kind == "sentinel"]:
        x = s.frame(sl.frame)
        for pair in range(s.route.pairs):
            lr = es.frame_lr(x, pair)
            assert np.array_equal(es.truth_frame(lr, s.route.W), oracle.np_truth_frame(lr, s.route.W)), (name, sl)


def test_zero_offsets_of_the_window():
    # Z: offset 0 up to W 19200; 0 .. 2 and W - 2 .. W - 1 at W 65536; the first 41 and last 40 at 2^20
    assert es.zero_offsets(2048) == es.zero_offsets(19200)[:1] == (0,)
    assert es.zero_offsets(65536) == (0, 1, 2, 65534, 65535)
    Z = es.zero_offsets(1 << 20)
    assert Z == tuple(range(41)) + tuple(range((1 << 20) - 40, 1 << 20))


def test_large_plan_restatement_matches_the_header(tmp_path):
    # the N2 of the column crossings and the chunk boundaries come from large_plan.hpp itself
    src = tmp_path / "plan.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "large_plan.hpp"\nusing namespace sgx::large;\n'
                   "int main(int argc, char **argv) { for (int i = 1; i < argc; ++i) { Plan p; uint32_t W = (uint32_t)atoi(argv[i]);\n"
                   "  if (!make_plan(W, p)) return 1; size_t c = kScratchBytes / scratch_per_transform(p); c = c < 1 ? 1 : c > 65535 ? 65535 : c;\n"
                   '  printf("%u %u %u %u %d %zu\\n", W, p.L, p.N1, p.N2, (int)p.chirp, c); } return 0; }\n')
    exe = str(tmp_path / "plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "spectrogram_rs_amd", "csrc"), str(src), "-o", exe], check=True,
                   timeout=300)
    Ws = sorted({r.W for r in es.ROUTES if r.kernel == 11})
    out = subprocess.run([exe] + [str(W) for W in Ws], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    for W, line in zip(Ws, out):
        L, N1, N2, chirp = es.large_plan(W)
        assert line.split() == [str(v) for v in (W, L, N1, N2, int(chirp), es.large_chunk(W))], line
