"""Rates of sgx_stft_batch_complex (complex (L, R) rows, 16 bytes per bin) beside sgx_stft_batch (magnitude pairs, 8 bytes per bin) on the
same context and stream, timed alternately in one process.  One JSON line per shape and output: frames per second and the fraction of
the 8 TB/s HBM roofline on ALGORITHMIC bytes (new input samples + the rows).

    python tools/complex_bench.py [--iters 10] [--warmup 2] [--case w2048_h256_lr ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
CASES = {   # name: (W, H, channels, frames, engine flags)
    "w2048_h256_mono": (2048, 256, 1, 1_000_000, {}),
    "w2048_h256_lr": (2048, 256, 2, 500_000, {}),
    "w2400_h93_lr": (2400, 93, 2, 262_144, {}),
    "w8192_h512_ch8": (8192, 512, 8, 16_384, {}),
    "w19200_h4800_lr_large": (19200, 4800, 2, 8_192, {"large_transforms": True}),
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
        W, H, ch, frames, flags = CASES[name]
        eng = SpectrogramEngine(48000.0, window_samples=W, hop_samples=H, channels=ch, device=0, **flags)
        pcm = eng.white_noise(W + (frames - 1) * H, seed=7)
        M, pairs = eng.M, eng.pairs
        mags = torch.empty((frames, pairs, M, 2), dtype=torch.float32, device=eng.device)
        spec = torch.empty((frames, pairs, M, 2), dtype=torch.complex64, device=eng.device)
        variants = {
            "complex": (lambda: eng.stft_batch_complex(pcm, out=spec), pairs * M * 16),
            "magnitudes": (lambda: eng.stft_batch(pcm, out=mags), pairs * M * 8),
        }
        for run, _ in variants.values():
            for _ in range(a.warmup):
                run()
        torch.cuda.synchronize()
        total = {k: 0.0 for k in variants}
        for _ in range(a.iters):
            for k, (run, _) in variants.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run()
                t1.record()
                torch.cuda.synchronize()
                total[k] += t0.elapsed_time(t1) / 1e3
        for k, (_, out_bytes) in variants.items():
            sec = total[k] / a.iters
            alg = H * ch * 4 + out_bytes
            print(json.dumps({"case": name, "output": k, "W": W, "H": H, "channels": ch, "frames": frames,
                              "stft_kernel": eng.info.stft_kernel, "render_path": eng.info.render_path, "ms": round(sec * 1e3, 4),
                              "M_frames_per_s": round(frames / sec / 1e6, 3), "alg_bytes_per_frame": alg,
                              "frac_of_roofline": round(alg * frames / sec / HBM_BYTES_PER_S, 4)}), flush=True)
        del pcm, mags, spec
        eng.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
