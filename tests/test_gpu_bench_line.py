"""bench.py's N = 1 run on the GPU, at reduced sizes, inside the suite the driver runs: ONE stdout line that parses, is at most 4 096 bytes
(the 21 KB line of that round was not parsed) and carries the contract keys -- with `roofline` and `cpu_baseline` under
--full, the headline alone without it; the full record on stderr and in bench_legs.json.  A fresh child process (this pytest process has
touched the GPU and is never replaced)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_the_full_run_prints_one_parsable_line_within_its_budget(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "BENCH_LAUNCH_ONLY", "BENCH_BACKEND", "BENCH_SINGLE_DEVICE", "BENCH_TEST_HOOKS"):
        env.pop(k, None)
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--frames", "65536", "--placements", "2", "--sustain-s", "0.2", "--leg-sustain-s", "0.1",
            "--pixel-frames", "65536", "--config4-hops", "2048", "--stereo-frames", "65536", "--paired-frames", "65536", "--complex-frames", "65536",
            "--app-frames", "16384", "--cpu-frames", "8192"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-3000:]                       # nothing else on stdout
    assert len(lines[0].encode()) <= 4096
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["metric"].startswith("STFT frames/sec") and line["unit"] == "frames/s" and line["n_gpus"] == 1 and line["steps"] == 3
    assert line["dtype"] == "f32" and line["vs_baseline"] is None and line["scaling"] == "weak" and line["higher_is_better"] is True
    assert line["config"]["workload"].startswith("configs[1]") and "model" not in line["config"]
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-5
    assert "traffic" in rf and rf["kernel"].startswith("sgx::")
    cb = line["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference") and cb["unit"] == "frames/s" and cb["sample"] and cb["parity_on_sample"] is True
    for k in ("config3_frac", "config4_frac", "stereo_frac"):
        assert 0 < line[k] < 1, k
    assert line["config3_rgba"]["stage_wise_bit_exact_on_128_frames"] is True and line["config3_rgba"]["max_lut_step"] <= 1
    # the full record: on stderr, and beside bench.py
    legs = [ln for ln in p.stderr.splitlines() if ln.startswith("bench_legs ")]
    assert len(legs) == 1
    full = json.loads(legs[0][len("bench_legs "):])
    assert full["value"] == line["value"] and "config4" in full and "placement" in full["roofline"]
    assert json.load(open(os.path.join(ROOT, "bench_legs.json")))["value"] == line["value"]


def test_a_plain_run_prints_the_headline_alone():
    # what is run for every change, several times: set-up, warm-up, the timed steps and the line -- no side leg, no CPU baseline,
    # no timed run of its own beside the headline
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "BENCH_LAUNCH_ONLY", "BENCH_BACKEND", "BENCH_SINGLE_DEVICE", "BENCH_TEST_HOOKS"):
        env.pop(k, None)
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "65536", "--placements", "2", "--sustain-s", "0.2"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0].encode()) <= 4096, p.stdout[-3000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline"):
        assert k in line, k
    assert line["metric"].startswith("STFT frames/sec") and line["unit"] == "frames/s" and line["steps"] == 3 and line["warmup"] == 1
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0 and line["ms_per_step"] > 0
    rf = line["roofline"]
    assert 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-5 and "measured_device" not in rf
    legs = [ln for ln in p.stderr.splitlines() if ln.startswith("bench_legs ")]
    assert len(legs) == 1
    full = json.loads(legs[0][len("bench_legs "):])
    for k in ("cpu_baseline", "config3", "config4", "stereo4096", "mono_paired_frames", "mono_complex_frames", "app_point", "config5"):
        assert k not in full, k
    assert full["value"] == line["value"] and full["roofline"]["measured_device"] is None and full["roofline"]["placement"]["candidates"] == 2
    # the first allocation is reported only where it costs no run of its own: when it is the buffer the timed steps wrote
    assert (full["roofline"]["first_allocation"] is None) == (full["roofline"]["placement"]["chosen"] != 0)


def test_dump_outputs_writes_the_last_timed_step(tmp_path, mags_err):
    import numpy as np

    import oracle
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "BENCH_LAUNCH_ONLY", "BENCH_BACKEND", "BENCH_SINGLE_DEVICE", "BENCH_TEST_HOOKS"):
        env.pop(k, None)
    F, W, H = 65536, 2048, 256
    out = tmp_path / "dump"
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", str(F), "--placements", "1", "--sustain-s", "0", "--pixel-frames", "0",
            "--config4-hops", "0", "--stereo-frames", "0", "--paired-frames", "0", "--complex-frames", "0", "--app-frames", "0", "--cpu-frames", "0",
            "--dump-outputs", str(out)]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert sorted(os.listdir(out)) == ["stft_frame_index.npy", "stft_mags.npy"]
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    mags, idx = np.load(out / "stft_mags.npy"), np.load(out / "stft_frame_index.npy")
    assert mags.dtype == np.float32 and idx.dtype == np.float64 and mags.shape == (len(idx), 1, W - 1, 2)
    assert idx[0] == 0 and idx[-1] == F - 1 and (np.diff(idx) > 0).all()
    for j in (0, 1, len(idx) // 2, len(idx) - 1):                # each dumped frame is its frame of the bench's stream
        t = int(idx[j])
        ref = oracle.stream_process(oracle.white_noise(W, first=t * H), 1, W, H)
        assert mags_err(mags[j:j + 1], ref) <= 2.0, t           # two float32 FFTs: 2 x the float32 bound, as in smoke()
