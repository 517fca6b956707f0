"""Rates of the multi-pass transform (SGX_FLAG_LARGE_TRANSFORM, stft_kernel 11): transforms per second and the fraction of the 8 TB/s
HBM roofline on ALGORITHMIC bytes (new input samples + output rows; the scratch round trips are not counted), one JSON line per case.

    python tools/large_bench.py [--frames 512] [--iters 20] [--warmup 3] [--case w19200_stereo ...]

Per-pass kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/large_bench.py --iters 5`; the bytes
the passes really move: a separate `rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d <dir> -- python tools/large_bench.py --iters 2`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
CASES = {   # name: (sample rate, W, H, channels)
    "w19200_stereo": (384000.0, 19200, 4800, 2),    # the application's 0.05 s at 384 kHz, 2W = 38400 (direct)
    "w16384_mono": (48000.0, 16384, 4096, 1),       # 2W = 32768 (direct), every frame its own (s, s) transform
    "w6001_stereo": (48000.0, 6001, 1500, 2),       # 2W = 2 17 353: chirp-z over L = 32768
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    a = ap.parse_args()

    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    for name in a.case or list(CASES):
        sr, W, H, ch = CASES[name]
        eng = SpectrogramEngine(sr, window_samples=W, hop_samples=H, channels=ch, device=0, large_transforms=True)
        assert eng.info.stft_kernel == 11, name
        n_samples = W + (a.frames - 1) * H
        pcm = eng.white_noise(n_samples, seed=7)
        out = torch.empty((a.frames, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        for _ in range(a.warmup):
            eng.stft_batch(pcm, out=out)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            eng.stft_batch(pcm, out=out)
        t1.record()
        torch.cuda.synchronize()
        sec = t0.elapsed_time(t1) / 1e3 / a.iters
        transforms = a.frames * eng.pairs
        alg_bytes = a.frames * (H * ch * 4 + eng.pairs * eng.M * 8)
        print(json.dumps({"case": name, "W": W, "H": H, "channels": ch, "frames": a.frames, "ms_per_batch": round(sec * 1e3, 4),
                          "transforms_per_s": round(transforms / sec, 1), "alg_bytes_per_frame": alg_bytes // a.frames,
                          "frac_of_roofline": round(alg_bytes / sec / HBM_BYTES_PER_S, 4)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
