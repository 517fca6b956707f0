"""Rates of sgx_bands_batch (PCM to the rows' magnitude_in means): the fused kernel, the two-kernel route (SGX_FLAG_NO_FUSED_RENDER) and
sgx_render_batch's RGBA on the same stream, timed interleaved on one device.  One JSON line per workload and variant: frames per second
and the fraction of the 8 TB/s HBM roofline on ALGORITHMIC bytes (new input samples + the output; the two-kernel route's magnitude
round trip is not counted).

    python tools/bands_bench.py [--iters 10] [--warmup 2] [--case config3_cubic ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
CASES = {   # name: (W, H, channels, interp, frames)
    "config3_cubic": (2048, 256, 1, 0, 1_000_000),
    "config3_cosine": (2048, 256, 1, 1, 1_000_000),
    "app_w2400_h93_lr": (2400, 93, 2, 0, 262_144),
    "w8192_h512_mono": (8192, 512, 1, 0, 65_536),
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
        W, H, ch, interp, frames = CASES[name]
        kw = dict(window_samples=W, hop_samples=H, channels=ch, interp=interp, device=0)
        fused, split = SpectrogramEngine(48000.0, **kw), SpectrogramEngine(48000.0, fused_render=False, **kw)
        pcm = fused.white_noise(W + (frames - 1) * H, seed=7)
        bands = torch.empty((frames, fused.pairs, fused.R, 2), dtype=torch.float32, device=fused.device)
        rgba = torch.empty((frames, fused.pairs, fused.R, 4), dtype=torch.uint8, device=fused.device)
        variants = {
            "bands_fused": (lambda: fused.bands_batch(pcm, out=bands), fused.pairs * fused.R * 8),
            "bands_two_kernel": (lambda: split.bands_batch(pcm, out=bands), fused.pairs * fused.R * 8),
            "rgba_render": (lambda: fused.render_batch(pcm, out=rgba), fused.pairs * fused.R * 4),
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
            print(json.dumps({"case": name, "variant": k, "W": W, "H": H, "channels": ch, "interp": "cosine" if interp else "cubic",
                              "frames": frames, "bands_fused": fused.bands_fused, "stft_kernel": fused.info.stft_kernel,
                              "ms": round(sec * 1e3, 4), "frames_per_s": round(frames / sec, 1), "alg_bytes_per_frame": alg,
                              "frac_of_roofline": round(alg * frames / sec / HBM_BYTES_PER_S, 4)}), flush=True)
        del pcm, bands, rgba
        fused.close()
        split.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
