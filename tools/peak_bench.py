"""Rates of sgx_bands_peak_batch (PCM to peak-hold band columns over groups of frames): the fused route, the workspace route
(SGX_FLAG_NO_FUSED_RENDER) and sgx_bands_batch's fused kernel on the same stream -- the unchanged code the peak columns are defined
by -- timed interleaved on one device, every iteration kept.  One JSON line per workload and leg: the median rate, the spread of the
iterations (p10 .. p90 and min .. max, as rates) and the bytes the leg's output holds per frame.  The first `--settle` seconds of
iterations load the device and are not counted.

    python tools/peak_bench.py [--iters 150] [--settle 3] [--group 256] [--case config3_cubic ...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = {   # name: (W, H, channels, interp, frames)
    "config3_cubic": (2048, 256, 1, 0, 1_000_000),
    "config3_cosine": (2048, 256, 1, 1, 1_000_000),
    "w2048_h256_lr": (2048, 256, 2, 0, 1_000_000),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--settle", type=float, default=3.0, help="seconds of interleaved iterations before the counted ones")
    ap.add_argument("--group", type=int, default=256)
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--once", action="store_true", help="one call of every leg per case and nothing else (for a counter pass: the kernels' names tell the legs apart)")
    a = ap.parse_args()

    import numpy as np
    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    for name in a.case or list(CASES):
        W, H, ch, interp, frames = CASES[name]
        kw = dict(window_samples=W, hop_samples=H, channels=ch, interp=interp, device=0)
        fused, split = SpectrogramEngine(48000.0, **kw), SpectrogramEngine(48000.0, fused_render=False, **kw)
        pcm = fused.white_noise(W + (frames - 1) * H, seed=7)
        cols = -(-frames // a.group)
        peak = torch.empty((cols, fused.pairs, fused.R, 2), dtype=torch.float32, device=fused.device)
        bands = torch.empty((frames, fused.pairs, fused.R, 2), dtype=torch.float32, device=fused.device)
        col_bytes = fused.pairs * fused.R * 8
        legs = {
            "peak_fused": (lambda: fused.bands_peak_batch(pcm, a.group, out=peak), col_bytes / a.group),
            "peak_workspace": (lambda: split.bands_peak_batch(pcm, a.group, out=peak), col_bytes / a.group),
            "bands_fused": (lambda: fused.bands_batch(pcm, out=bands), col_bytes),
        }

        if a.once:
            for run, _ in legs.values():
                run()
            torch.cuda.synchronize()
            continue

        def one_round():
            ms = {}
            for k, (run, _) in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run()
                t1.record()
                torch.cuda.synchronize()
                ms[k] = t0.elapsed_time(t1)
            return ms

        t_end = time.perf_counter() + a.settle
        one_round()
        while time.perf_counter() < t_end:
            one_round()
        rounds = [one_round() for _ in range(a.iters)]
        for k, (_, out_bytes) in legs.items():
            rate = np.sort(frames / (np.array([r[k] for r in rounds]) / 1e3))
            q = lambda f: float(rate[min(len(rate) - 1, int(f * len(rate)))])
            print(json.dumps({"case": name, "leg": k, "W": W, "H": H, "channels": ch, "interp": "cosine" if interp else "cubic",
                              "frames": frames, "group": a.group, "iters": a.iters, "bands_peak_fused": fused.bands_peak_fused,
                              "stft_kernel": fused.info.stft_kernel, "median_frames_per_s": round(q(0.5), 1),
                              "p10_frames_per_s": round(q(0.1), 1), "p90_frames_per_s": round(q(0.9), 1),
                              "min_frames_per_s": round(float(rate[0]), 1), "max_frames_per_s": round(float(rate[-1]), 1),
                              "spread_p10_p90_of_median": round((q(0.9) - q(0.1)) / q(0.5), 4),
                              "output_bytes_per_frame": round(out_bytes, 2)}), flush=True)
        del pcm, bands, peak
        fused.close()
        split.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
