"""Rates of sgx_fbank_batch (PCM to the sums of a 128-filter mel bank over the bin powers): the fused kernel and the workspace route
(SGX_FLAG_NO_FUSED_RENDER: the rows of a chunk of frames into the bounded workspace, then the stage kernel) timed alternately in one
process on one device, with sgx_bands_batch on the same stream beside them for scale.  Timed steps from device events after a warm-up;
one JSON line per workload and variant with every step's time, so that the spread between repeats of one leg is on the record:
frames per second from the median step, and the fraction of the 8 TB/s HBM roofline on ALGORITHMIC bytes, 4 H channels + 8 n_filters pairs
per frame (the workspace route's round trip of the rows is not counted).

    python tools/fbank_bench.py [--iters 10] [--warmup 2] [--frames 1000000] [--case mono ...]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
CASES = {"mono": 1, "lr": 2}   # name: channels, at W 2048 / H 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--mels", type=int, default=128)
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    a = ap.parse_args()

    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    W, H, frames = 2048, 256, a.frames
    for name in a.case or list(CASES):
        ch = CASES[name]
        kw = dict(window_samples=W, hop_samples=H, channels=ch, device=0)
        fused, split = SpectrogramEngine(48000.0, **kw), SpectrogramEngine(48000.0, fused_render=False, **kw)
        fb_fused, fb_split = fused.mel_filterbank(a.mels, power=2), split.mel_filterbank(a.mels, power=2)
        pcm = fused.white_noise(W + (frames - 1) * H, seed=7)
        sums = torch.empty((frames, fused.pairs, a.mels, 2), dtype=torch.float32, device=fused.device)
        bands = torch.empty((frames, fused.pairs, fused.R, 2), dtype=torch.float32, device=fused.device)
        variants = {
            "fbank_fused": (lambda: fb_fused.batch(pcm, out=sums), fused.pairs * a.mels * 8, fb_fused.fused),
            "fbank_workspace": (lambda: fb_split.batch(pcm, out=sums), fused.pairs * a.mels * 8, fb_split.fused),
            "bands_fused": (lambda: fused.bands_batch(pcm, out=bands), fused.pairs * fused.R * 8, fused.bands_fused),
        }
        for run, _, _ in variants.values():
            for _ in range(a.warmup):
                run()
        torch.cuda.synchronize()
        steps = {k: [] for k in variants}
        for _ in range(a.iters):
            for k, (run, _, _) in variants.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run()
                t1.record()
                torch.cuda.synchronize()
                steps[k].append(t0.elapsed_time(t1))
        for k, (_, out_bytes, one_kernel) in variants.items():
            ms = statistics.median(steps[k])
            alg = H * ch * 4 + out_bytes
            print(json.dumps({"case": name, "variant": k, "W": W, "H": H, "channels": ch, "frames": frames, "filters": a.mels if k != "bands_fused" else fused.R,
                              "weights": int(fb_fused._n_weights) if k != "bands_fused" else None, "one_kernel": one_kernel,
                              "ms_median": round(ms, 4), "ms_min": round(min(steps[k]), 4), "ms_max": round(max(steps[k]), 4),
                              "ms_steps": [round(x, 4) for x in steps[k]], "frames_per_s": round(frames / (ms / 1e3), 1),
                              "alg_bytes_per_frame": alg, "frac_of_roofline": round(alg * frames / (ms / 1e3) / HBM_BYTES_PER_S, 4)}), flush=True)
        del pcm, sums, bands
        fb_fused.close(), fb_split.close()
        fused.close()
        split.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
