"""Rates of sgx_istft_batch (PCM from complex (L, R) spectra by weighted overlap-add) on the spectra of sgx_stft_batch_complex, one
context and stream per shape.  One JSON line per shape: frames per second and the fraction of the 8 TB/s HBM roofline on ALGORITHMIC
bytes (the spectra, pairs (W - 1) 16 per frame, read + the new samples, H channels 4 per frame, written).

    python tools/istft_bench.py [--iters 10] [--warmup 2] [--case w2048_h256_lr ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
CASES = {   # name: (W, H, channels, frames)
    "w2048_h256_lr": (2048, 256, 2, 200_000),
    "w2048_h256_mono": (2048, 256, 1, 200_000),
    "w2400_h93_lr": (2400, 93, 2, 131_072),
    "w8192_h512_lr": (8192, 512, 2, 32_768),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    a = ap.parse_args()

    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    for name in a.case or list(CASES):
        W, H, ch, frames = CASES[name]
        eng = SpectrogramEngine(48000.0, window_samples=W, hop_samples=H, channels=ch, device=0)
        pcm = eng.white_noise(W + (frames - 1) * H, seed=7)
        spec = eng.stft_batch_complex(pcm)
        assert spec.shape[0] == frames
        out = torch.empty(((frames - 1) * H + W, ch), dtype=torch.float32, device=eng.device)
        for _ in range(a.warmup):
            eng.istft_batch(spec, out=out)
        torch.cuda.synchronize()
        total = 0.0
        for _ in range(a.iters):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            eng.istft_batch(spec, out=out)
            t1.record()
            torch.cuda.synchronize()
            total += t0.elapsed_time(t1) / 1e3
        sec = total / a.iters
        alg = eng.pairs * (W - 1) * 16 + H * ch * 4
        interior = slice(W, (frames - 1) * H)
        err = float((out[interior] - pcm.view(-1, ch)[interior]).abs().max())
        print(json.dumps({"case": name, "W": W, "H": H, "channels": ch, "frames": frames, "stft_kernel": eng.info.stft_kernel,
                          "ms": round(sec * 1e3, 4), "M_frames_per_s": round(frames / sec / 1e6, 3), "alg_bytes_per_frame": alg,
                          "frac_of_roofline": round(alg * frames / sec / HBM_BYTES_PER_S, 4), "round_trip_max_abs_err": err}), flush=True)
        del pcm, spec, out
        eng.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
