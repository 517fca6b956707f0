"""Rates of sgx_fbank_cross_batch (PCM to the sums of |L|^2, |R|^2, Re and Im of L conj R over a 128-filter mel bank) at W 2048 / H 256 on
an (l, r) stream: (a) the fused kernel, (b) the workspace route (SGX_FLAG_NO_FUSED_RENDER: the complex rows of a chunk of frames into the
bounded workspace, then the stage kernel), (c) sgx_stft_batch_complex alone -- what any caller-side reduction has to pay first, written
in chunks of --chunk frames into one buffer that is reused -- and (d) sgx_fbank_batch, the magnitude bank, beside them.  The legs are timed
alternately in one process on one device, from device events after a warm-up; one JSON line per leg with every step's time, so that the
spread between repeats of one leg is on the record: frames per second from the median step, and the fraction of the 8 TB/s HBM roofline
on ALGORITHMIC bytes, 8 H of samples plus the leg's output per frame (the workspace route's round trip of the rows is not counted).

    python tools/fbank_cross_bench.py [--iters 10] [--warmup 2] [--frames 1000000] [--chunk 65536]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--mels", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=65536, help="frames of complex rows per sgx_stft_batch_complex call of leg (c): 32 KB each")
    a = ap.parse_args()

    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    W, H, ch, frames = 2048, 256, 2, a.frames
    kw = dict(window_samples=W, hop_samples=H, channels=ch, device=0)
    fused, split = SpectrogramEngine(48000.0, **kw), SpectrogramEngine(48000.0, fused_render=False, **kw)
    fb_fused, fb_split = fused.mel_filterbank(a.mels, power=2), split.mel_filterbank(a.mels, power=2)
    pcm = fused.white_noise(W + (frames - 1) * H, seed=7)
    cross = torch.empty((frames, fused.pairs, a.mels, 4), dtype=torch.float32, device=fused.device)
    sums = torch.empty((frames, fused.pairs, a.mels, 2), dtype=torch.float32, device=fused.device)
    chunk = min(a.chunk, frames)
    rows = torch.empty((chunk, fused.pairs, fused.M, 2, 2), dtype=torch.float32, device=fused.device)

    def complex_rows():
        for first in range(0, frames, chunk):
            n = min(chunk, frames - first)
            fused.stft_batch_complex(pcm, first_frame=first, max_frames=n, out=rows[:n])

    row_bytes = fused.pairs * fused.M * 16
    variants = {
        "a_cross_fused": (lambda: fb_fused.cross_batch(pcm, out=cross), fused.pairs * a.mels * 16, fb_fused.cross_fused),
        "b_cross_workspace": (lambda: fb_split.cross_batch(pcm, out=cross), fused.pairs * a.mels * 16, fb_split.cross_fused),
        "c_complex_rows": (complex_rows, row_bytes, 1),
        "d_fbank_fused": (lambda: fb_fused.batch(pcm, out=sums), fused.pairs * a.mels * 8, fb_fused.fused),
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
        print(json.dumps({"variant": k, "W": W, "H": H, "channels": ch, "frames": frames, "filters": a.mels if k != "c_complex_rows" else None,
                          "weights": int(fb_fused._n_weights) if k != "c_complex_rows" else None, "one_kernel": one_kernel,
                          "chunk_frames": chunk if k == "c_complex_rows" else None,
                          "ms_median": round(ms, 4), "ms_min": round(min(steps[k]), 4), "ms_max": round(max(steps[k]), 4),
                          "ms_steps": [round(x, 4) for x in steps[k]], "frames_per_s": round(frames / (ms / 1e3), 1),
                          "alg_bytes_per_frame": alg, "frac_of_roofline": round(alg * frames / (ms / 1e3) / HBM_BYTES_PER_S, 4)}), flush=True)
    fb_fused.close(), fb_split.close()
    fused.close()
    split.close()


if __name__ == "__main__":
    main()
