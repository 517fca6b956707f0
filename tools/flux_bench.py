"""Rates of sgx_flux_batch (PCM to the per-band sums of every bin's rise and fall against the frame `lag` earlier, over a 128-filter
mel bank at power 2) at W 2048 / H 256, lag 1 and 8, on a mono and on an (l, r) stream: (a) the call -- the rows of a range through the
192 MiB workspace, then the flux stage; (b) sgx_fbank_batch on the same bank and stream, fused; (c) the same with
SGX_FLAG_NO_FUSED_RENDER, the workspace route: the flux call's own shape without the second row and the two extra chains; (d) the same
result from rows stored in chunks of --chunk-bytes (the `lag` rows before a chunk stored again) and reduced with torch -- square, shifted
subtract, two clamps, a dense matrix product; (e) that row store alone.  The legs are timed alternately in one process on one device, from
device events after a warm-up; one JSON line per leg with every step's time, so that the spread between repeats of one leg is on the record.

    python tools/flux_bench.py [--iters 10] [--warmup 2] [--frames 1000000] [--chunk-bytes 2147483648]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--mels", type=int, default=128)
    ap.add_argument("--chunk-bytes", type=int, default=2 << 30)
    ap.add_argument("--lags", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()

    import numpy as np
    import torch
    from spectrogram_rs_amd import SpectrogramEngine, mel_weights

    W, H, frames = 2048, 256, a.frames
    for ch in (1, 2):
        kw = dict(window_samples=W, hop_samples=H, channels=ch, device=0)
        fused, split = SpectrogramEngine(48000.0, **kw), SpectrogramEngine(48000.0, fused_render=False, **kw)
        first, count, weights = mel_weights(48000.0, W, a.mels, 0.0, 24000.0)
        fb, fb_split = fused.filterbank(first, count, weights, power=2), split.filterbank(first, count, weights, power=2)
        assert fb.fused == 1 and fb_split.fused == 0
        pcm = fused.white_noise(W + (frames - 1) * H, seed=7)
        flux = torch.empty((frames, fused.pairs, a.mels, 4), dtype=torch.float32, device=fused.device)
        sums = torch.empty((frames, fused.pairs, a.mels, 2), dtype=torch.float32, device=fused.device)
        row_bytes = fused.pairs * fused.M * 8
        chunk = max(1, min(a.chunk_bytes // row_bytes - max(a.lags), frames))
        rows = torch.empty((chunk + max(a.lags), fused.pairs, fused.M, 2), dtype=torch.float32, device=fused.device)
        dense = np.zeros((a.mels, fused.M), np.float32)
        off = 0
        for f in range(a.mels):
            dense[f, first[f]:first[f] + count[f]] = weights[off:off + count[f]]
            off += int(count[f])
        dense = torch.from_numpy(dense).to(fused.device)

        def store(lag, reduce):
            for start in range(0, frames, chunk):
                n = min(chunk, frames - start)
                back = min(lag, start)
                r = rows[:back + n]
                fused.stft_batch(pcm, first_frame=start - back, max_frames=back + n, out=r)
                if not reduce:
                    continue
                x = r * r
                d = x[lag:] - x[:-lag]
                out = flux[start:start + n]
                if back < lag:                                               # the call's first chunk: frames t < lag are zero
                    out[:lag - back] = 0.0
                    out = out[lag - back:]
                out[..., :2] = torch.matmul(dense, d.clamp(min=0.0))
                out[..., 2:] = torch.matmul(dense, (-d).clamp(min=0.0))

        variants = {}
        for lag in a.lags:
            variants[f"a_flux_lag{lag}"] = (lambda lag=lag: fb.flux_batch(pcm, lag=lag, out=flux), lag)
        variants["b_fbank_fused"] = (lambda: fb.batch(pcm, out=sums), None)
        variants["c_fbank_workspace"] = (lambda: fb_split.batch(pcm, out=sums), None)
        for lag in a.lags:
            variants[f"d_store_reduce_torch_lag{lag}"] = (lambda lag=lag: store(lag, True), lag)
        variants["e_row_store"] = (lambda: store(max(a.lags), False), max(a.lags))
        # the torch reduction gives the call's result up to the order of its sums (looked at on the call's last frames)
        for lag in a.lags:
            tail = fb.flux_batch(pcm, lag=lag, first_frame=max(frames - 64, 0))
            store(lag, True)
            err = float((flux[-tail.shape[0]:] - tail).abs().max() / tail.abs().max())
            assert err < 1e-4, (lag, err)
        for run, _ in variants.values():
            for _ in range(a.warmup):
                run()
        torch.cuda.synchronize()
        steps = {k: [] for k in variants}
        for _ in range(a.iters):
            for k, (run, _) in variants.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run()
                t1.record()
                torch.cuda.synchronize()
                steps[k].append(t0.elapsed_time(t1))
        for k, (_, lag) in variants.items():
            ms = statistics.median(steps[k])
            print(json.dumps({"variant": k, "W": W, "H": H, "channels": ch, "frames": frames, "filters": a.mels, "lag": lag,
                              "chunk_frames": chunk if k[0] in "de" else None,
                              "ms_median": round(ms, 4), "ms_min": round(min(steps[k]), 4), "ms_max": round(max(steps[k]), 4),
                              "spread_pct": round(100.0 * (max(steps[k]) - min(steps[k])) / ms, 2),
                              "ms_steps": [round(x, 4) for x in steps[k]], "frames_per_s": round(frames / (ms / 1e3), 1)}), flush=True)
        fb.close(), fb_split.close()
        fused.close()
        split.close()
        del rows, flux, sums, pcm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
